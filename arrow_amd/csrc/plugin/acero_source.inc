// The table_source_rocm Acero exec node.
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- Acero: a table source sized for a GPU
// TableSourceNode (acero/source_node.cc:303-378) turns a Table into morsels of max_batch_size rows and SourceNode
// (source_node.cc:122-160) slices every morsel into ExecBatches of ExecPlan::kMaxBatchSize = 32Ki rows, the size of a
// CPU core's L2.  Downstream every node then runs once per 32Ki rows: FilterNode evaluates its predicate and calls
// Filter per column (filter_node.cc:73-108), ProjectNode evaluates its expressions — over device-resident columns that
// is a handful of kernel launches and a count readback per 32Ki rows, ~8000 times for 2^28 rows, where ONE launch per
// column covers the whole table in a few hundred microseconds.  This source delivers a device table in batches of
// max_batch_size rows WITHOUT the 32Ki slicing (one batch per chunk when the chunks are smaller), so the stock
// FilterNode / ProjectNode — which take batches of any length — and aggregate_rocm / order_by_rocm run once per batch
// through the kernels this shim registered.  Same options class, same validation, same implicit ordering and batch
// indices as the reference node; registered under a NEW name (duplicates are rejected, acero/exec_plan.cc:1132-1142).
// TableSourceNodeOptions::max_batch_size left at its default (1Mi rows, options.h kDefaultTableSourceNodeMaxBatchSize)
// is replaced by the plugin's table_source_rows (2^27): the default was chosen for host memory.
// Nodes that index rows with 16 bits (the hash join's) must not sit downstream of this source.  The guard in
// plugin/acero_override.inc keeps the stock `hashjoin` away from it: a join with a remembered device source among its
// inputs is built as hashjoin_rocm (plugin/hash_join_node.inc) or refused with a Status.
class RocmTableSourceNode : public ac::ExecNode {
 public:
  RocmTableSourceNode(ac::ExecPlan* plan, std::shared_ptr<arrow::Table> table, int64_t batch_rows)
      : ac::ExecNode(plan, {}, {}, table->schema()), table_(std::move(table)), batch_rows_(batch_rows) {}

  static arrow::Result<ac::ExecNode*> Make(ac::ExecPlan* plan, std::vector<ac::ExecNode*> inputs,
                                           const ac::ExecNodeOptions& options) {
    if (!inputs.empty()) return Status::Invalid("TableSourceNode requires 0 inputs, but got ", inputs.size());
    const auto* opts = dynamic_cast<const ac::TableSourceNodeOptions*>(&options);
    if (opts == nullptr) return Status::TypeError("table_source_rocm expects TableSourceNodeOptions");
    if (opts->table == nullptr) return Status::Invalid("TableSourceNode requires table which is not null");
    if (opts->max_batch_size <= 0) {
      return Status::Invalid("TableSourceNode node requires, batch_size > 0 , but got batch size ", opts->max_batch_size);
    }
    const int64_t rows = opts->max_batch_size == ac::TableSourceNodeOptions::kDefaultMaxBatchSize
                             ? std::max<int64_t>(g_table_source_rows.load(), 1)
                             : opts->max_batch_size;
    return plan->EmplaceNode<RocmTableSourceNode>(plan, opts->table, rows);
  }

  const char* kind_name() const override { return "RocmTableSourceNode"; }
  const cp::Ordering& ordering() const override { return cp::Ordering::Implicit(); }

  Status InputReceived(ac::ExecNode*, cp::ExecBatch) override { return Status::Invalid("a source node has no inputs"); }
  Status InputFinished(ac::ExecNode*, int) override { return Status::Invalid("a source node has no inputs"); }
  void PauseProducing(ac::ExecNode*, int32_t) override {}     // (few, large batches: nothing to throttle)
  void ResumeProducing(ac::ExecNode*, int32_t) override {}

  Status StartProducing() override {
    // one task delivers every batch in order: the work per batch is kernel launches on this thread's stream, and the
    // nodes downstream serialise on the device anyway
    plan_->query_context()->ScheduleTask(
        [this]() -> Status {
          arrow::TableBatchReader reader(*table_);
          reader.set_chunksize(batch_rows_);
          int count = 0;
          for (;;) {
            if (stopped_.load()) break;
            std::shared_ptr<arrow::RecordBatch> batch;
            ARROW_RETURN_NOT_OK(reader.ReadNext(&batch));
            if (batch == nullptr) break;
            cp::ExecBatch exec_batch(*batch);
            exec_batch.index = count++;
            ARROW_RETURN_NOT_OK(output_->InputReceived(this, std::move(exec_batch)));
          }
          return output_->InputFinished(this, count);
        },
        "RocmTableSourceNode::Deliver");
    return Status::OK();
  }

 protected:
  Status StopProducingImpl() override {
    stopped_.store(true);
    return Status::OK();
  }

 private:
  std::shared_ptr<arrow::Table> table_;
  int64_t batch_rows_;
  std::atomic<bool> stopped_{false};
};

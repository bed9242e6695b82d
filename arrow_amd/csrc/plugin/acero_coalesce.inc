// The coalesce_rocm Acero exec node.
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- Acero: morsels -> a few large batches
// For plans whose source cannot be table_source_rocm (a scan, a user's source node, the stock table_source): every
// node of Acero runs once per ExecBatch and the sources cut batches of ExecPlan::kMaxBatchSize = 32Ki rows
// (acero/source_node.cc:122-160) — over device-resident columns FilterNode / ProjectNode (filter_node.cc:73-108) then
// pay a handful of launches and a count read-back 8192 times for 2^28 rows (1.8 s against 12 ms).  This node gathers its
// input and hands it on as batches of at least `coalesce_rows` rows (2^26; arrow_amd_plugin_set_coalesce_rows), in the
// order of the batch indices: Concatenate per column on the device (ConcatOnDevice — consecutive
// slices of one device array, which is what table_source makes of a device table, are re-joined without a copy).
// It waits for the end of its input (an AccumulatingNode, like the order-by and aggregate nodes it usually feeds).
// Host-resident batches pass through untouched: coalescing them would move them to the device behind the caller's back.
// No options of its own (any ExecNodeOptions object is accepted and ignored); registered under a NEW name.
class RocmCoalesceNode : public AccumulatingNode {
 public:
  RocmCoalesceNode(ac::ExecPlan* plan, std::vector<ac::ExecNode*> inputs, std::shared_ptr<arrow::Schema> schema)
      : AccumulatingNode(plan, std::move(inputs), {"input"}, std::move(schema)) {}

  static arrow::Result<ac::ExecNode*> Make(ac::ExecPlan* plan, std::vector<ac::ExecNode*> inputs, const ac::ExecNodeOptions&) {
    if (inputs.size() != 1) return Status::Invalid("coalesce_rocm takes exactly one input");
    for (const auto& f : inputs[0]->output_schema()->fields()) {
      const auto& t = *f->type();
      if (FixedByteWidth(t) == 0 && t.id() != Type::BOOL && !IsInt32Binary(t)) {
        return Status::NotImplemented("coalesce_rocm: column of type ", t.ToString());
      }
    }
    auto schema = inputs[0]->output_schema();
    return plan->EmplaceNode<RocmCoalesceNode>(plan, std::move(inputs), std::move(schema));
  }

  const char* kind_name() const override { return "RocmCoalesceNode"; }
  const cp::Ordering& ordering() const override { return inputs_[0]->ordering(); }

 private:
  static bool AllDeviceArrays(const cp::ExecBatch& b) {
    for (const auto& v : b.values) {
      if (!v.is_array() || !DataOnRocm(*v.array())) return false;
    }
    return !b.values.empty();
  }

  Status Finish() override {
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    std::vector<cp::ExecBatch>& batches = batches_[0];
    OrderBatchesByIndex(&batches);
    const int64_t target = std::max<int64_t>(g_coalesce_rows.load(), 1);
    const int ncols = output_schema()->num_fields();
    int emitted = 0;
    size_t i = 0;
    while (i < batches.size()) {
      if (!AllDeviceArrays(batches[i])) {   // host rows (or scalar columns): handed on as they came
        cp::ExecBatch b = std::move(batches[i++]);
        b.index = emitted++;
        ARROW_RETURN_NOT_OK(output_->InputReceived(this, std::move(b)));
        continue;
      }
      size_t j = i;
      int64_t rows = 0;
      while (j < batches.size() && AllDeviceArrays(batches[j]) && (rows < target || j == i)) rows += batches[j++].length;
      if (j == i + 1) {
        cp::ExecBatch b = std::move(batches[i]);
        b.index = emitted++;
        ARROW_RETURN_NOT_OK(output_->InputReceived(this, std::move(b)));
      } else {
        std::vector<arrow::Datum> columns(ncols);
        for (int c = 0; c < ncols; ++c) {
          std::vector<std::shared_ptr<ArrayData>> chunks;
          chunks.reserve(j - i);
          for (size_t k = i; k < j; ++k) chunks.push_back(batches[k].values[c].array());
          ARROW_ASSIGN_OR_RAISE(auto joined, ConcatOnDevice(output_schema()->field(c)->type(), chunks, st));
          columns[c] = arrow::Datum(std::move(joined));
        }
        cp::ExecBatch out(std::move(columns), rows);
        out.index = emitted++;
        g_coalesced_batches.fetch_add(static_cast<int64_t>(j - i));
        ARROW_RETURN_NOT_OK(output_->InputReceived(this, std::move(out)));
      }
      i = j;
    }
    batches.clear();
    return output_->InputFinished(this, emitted);
  }
};

// The aggregate_rocm Acero exec node (fused device group-by).
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- Acero: fused group-by node
// Whole-operator replacement (SURVEY.md 8b): an ExecNode registered with
// default_exec_factory_registry()->AddFactory("aggregate_rocm", ...) (acero/exec_plan.h:353-373;
// names must be new, exec_plan.cc:1132-1142) that takes the place of GroupByNode
// (acero/groupby_aggregate_node.cc:210-337) for `hash_sum(int64) GROUP BY int32`: instead of a CPU
// Grouper feeding dense ids to the aggregate kernel, keys and values go to the fused device
// operator (arx_groupby_*: hash partition -> LDS tables -> HBM table).  Batches without nulls are
// appended to device staging buffers and consumed in ONE partitioned pass when the input ends; a batch
// with nulls is consumed on arrival (the node overrides AccumulatingNode::Accept and keeps no batch).  Output = key column ++ aggregate column like
// GroupByNode::Finalize (:300-333), row order unspecified (as the reference with threads).
class RocmGroupBySumNode : public AccumulatingNode {
 public:
  // one output column per requested aggregate; all of them read the same fused per-group state
  // (wrap-around sum, count of valid values, "a null value was seen")
  enum AggKind { kSum, kCount, kMin, kMax, kMean };
  struct AggSpec {
    AggKind kind = kSum;                 // hash_sum | hash_count (ONLY_VALID) | hash_min | hash_max | hash_mean
    cp::ScalarAggregateOptions options;  // sum: skip_nulls / min_count; min/max: skip_nulls
  };

  RocmGroupBySumNode(ac::ExecPlan* plan, std::vector<ac::ExecNode*> inputs,
                     std::shared_ptr<arrow::Schema> out_schema, int key_idx, int val_idx,
                     std::vector<AggSpec> aggs)
      : AccumulatingNode(plan, std::move(inputs), {"input"}, std::move(out_schema)),
        key_idx_(key_idx), val_idx_(val_idx), aggs_(std::move(aggs)) {
    for (const auto& a : aggs_) needs_minmax_ = needs_minmax_ || a.kind == kMin || a.kind == kMax || a.kind == kMean;
  }

  ~RocmGroupBySumNode() override {
    // (the table and the staging columns are pooled device buffers: released with their shared_ptr)
  }

  static arrow::Result<ac::ExecNode*> Make(ac::ExecPlan* plan, std::vector<ac::ExecNode*> inputs,
                                           const ac::ExecNodeOptions& options) {
    if (inputs.size() != 1) return Status::Invalid("aggregate_rocm takes exactly one input");
    const auto* opts = dynamic_cast<const ac::AggregateNodeOptions*>(&options);
    if (opts == nullptr) return Status::TypeError("aggregate_rocm expects AggregateNodeOptions");
    if (opts->keys.size() != 1 || !opts->segment_keys.empty() || opts->aggregates.empty()) {
      return Status::NotImplemented("aggregate_rocm: one key, no segment keys, at least one aggregate");
    }
    const auto& in_schema = *inputs[0]->output_schema();
    ARROW_ASSIGN_OR_RAISE(auto kpath, opts->keys[0].FindOne(in_schema));
    if (kpath.indices().size() != 1) return Status::NotImplemented("aggregate_rocm: nested field references");
    const int ki = kpath[0];
    int vi = -1;
    std::vector<AggSpec> aggs;
    std::vector<std::shared_ptr<arrow::Field>> fields{in_schema.field(ki)};
    for (const auto& agg : opts->aggregates) {
      AggSpec spec;
      if (agg.function == "hash_min" || agg.function == "hash_max") {
        spec.kind = agg.function == "hash_min" ? kMin : kMax;
        if (agg.options != nullptr) {
          const auto* so = dynamic_cast<const cp::ScalarAggregateOptions*>(agg.options.get());
          if (so == nullptr) return Status::TypeError("aggregate_rocm: ", agg.function, " takes ScalarAggregateOptions");
          spec.options = *so;
        }
      } else if (agg.function == "hash_count") {
        spec.kind = kCount;
        if (agg.options != nullptr) {
          const auto* co = dynamic_cast<const cp::CountOptions*>(agg.options.get());
          if (co == nullptr) return Status::TypeError("aggregate_rocm: hash_count takes CountOptions");
          if (co->mode != cp::CountOptions::ONLY_VALID) {
            return Status::NotImplemented("aggregate_rocm: hash_count with CountOptions::ONLY_VALID only");
          }
        }
      } else if (agg.function == "hash_sum" || agg.function == "hash_mean") {
        if (agg.function == "hash_mean") spec.kind = kMean;
        if (agg.options != nullptr) {
          const auto* so = dynamic_cast<const cp::ScalarAggregateOptions*>(agg.options.get());
          if (so == nullptr) return Status::TypeError("aggregate_rocm: ", agg.function, " takes ScalarAggregateOptions");
          spec.options = *so;
        }
      } else {
        return Status::NotImplemented("aggregate_rocm: hash_sum / hash_mean / hash_count / hash_min / hash_max only, got ",
                                      agg.function);
      }
      if (agg.target.size() != 1) return Status::NotImplemented("aggregate_rocm: unary aggregates only");
      ARROW_ASSIGN_OR_RAISE(auto vpath, agg.target[0].FindOne(in_schema));
      if (vpath.indices().size() != 1) return Status::NotImplemented("aggregate_rocm: nested field references");
      if (vi >= 0 && vpath[0] != vi) {
        return Status::NotImplemented("aggregate_rocm: all aggregates must read the same value column");
      }
      vi = vpath[0];
      aggs.push_back(spec);
      fields.push_back(arrow::field(agg.name, spec.kind == kMean ? arrow::float64() : arrow::int64()));
    }
    if (in_schema.field(ki)->type()->id() != Type::INT32 || in_schema.field(vi)->type()->id() != Type::INT64) {
      return Status::NotImplemented("aggregate_rocm: hash_sum(int64) GROUP BY int32 only, got key ",
                                    in_schema.field(ki)->type()->ToString(), " value ",
                                    in_schema.field(vi)->type()->ToString());
    }
    return plan->EmplaceNode<RocmGroupBySumNode>(plan, std::move(inputs), arrow::schema(std::move(fields)), ki, vi,
                                                 std::move(aggs));
  }

  const char* kind_name() const override { return "RocmGroupBySumNode"; }

 private:
  // batches are consumed (or staged) as they arrive instead of being kept
  Status Accept(int, cp::ExecBatch batch) override {
    largest_input_batch_ = std::max(largest_input_batch_, batch.length);
    return Consume(batch);
  }

  static constexpr int64_t kMaxCapacity = int64_t(1) << 28;

  // {min, max} of the key slots of one device column folded into key_lo_ / key_hi_ (one pass over 4 B/row and an 8-byte
  // read-back): the groups are bounded by the rows AND by the width of the key range.  268M rows of 10M ids: a table of
  // 2^25 slots instead of 2^28 — 7 GB less to clear, to probe at random and to scan at the end.
  Status WidenKeyRange(const void* d_keys, int64_t offset, int64_t n, hipStream_t st) {
    if (n == 0) return Status::OK();
    void* d_range = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(kFlag, 64, &d_range));
    const int32_t init[2] = {INT32_MAX, INT32_MIN};
    int32_t got[2] = {0, 0};
    HIP_RETURN_NOT_OK(hipMemcpyAsync(d_range, init, 8, hipMemcpyHostToDevice, st));
    ArxSpan dk{nullptr, d_keys, offset, n, 0};
    ARROW_RETURN_NOT_OK(FromArx(arx_groupby_key_range_i32(&dk, static_cast<int32_t*>(d_range), st)));
    HIP_RETURN_NOT_OK(hipMemcpyAsync(got, d_range, 8, hipMemcpyDeviceToHost, st));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (init / got are locals)
    key_lo_ = std::min(key_lo_, got[0]);
    key_hi_ = std::max(key_hi_, got[1]);
    return Status::OK();
  }

  Status EnsureState(int64_t more_rows) {
    // capacity: a power of two above twice the distinct keys possible so far
    int64_t groups_bound = rows_seen_ + more_rows;
    if (key_range_complete_ && key_hi_ >= key_lo_) {   // every key so far lies in [key_lo_, key_hi_] (+ the null key's group)
      groups_bound = std::min<int64_t>(groups_bound, static_cast<int64_t>(key_hi_) - key_lo_ + 2);
    }
    const int64_t bound = std::min<int64_t>(kMaxCapacity, 2 * groups_bound + 2);
    int64_t cap = 1 << 16;
    while (cap < bound) cap <<= 1;
    if (state_ != nullptr && cap <= capacity_) return Status::OK();
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    // (pooled: a GB-sized hipMalloc per plan costs more than the whole aggregation)
    ARROW_ASSIGN_OR_RAISE(auto fresh_table, AllocAligned(static_cast<int64_t>(arx_groupby_state_bytes(cap))));
    AlignedDevice fresh_minmax{nullptr, nullptr};
    void* const fresh = fresh_table.ptr;
    ARROW_RETURN_NOT_OK(FromArx(arx_groupby_init(fresh, cap, st)));
    if (needs_minmax_) {
      ARROW_ASSIGN_OR_RAISE(fresh_minmax, AllocAligned(static_cast<int64_t>(arx_groupby_minmax_bytes(cap))));
      ARROW_RETURN_NOT_OK(FromArx(arx_groupby_minmax_init(fresh_minmax.ptr, cap, st)));
    }
    if (state_ != nullptr) {  // rehash: export the old table's partial aggregates, merge them
      int64_t g = 0;
      ARROW_RETURN_NOT_OK(FromArx(arx_groupby_num_groups(state_, &g, st)));
      if (g > 0) {
        void *k, *kv, *s, *c, *nn;
        ARROW_RETURN_NOT_OK(t_scratch.Get(kValues, g * 4 + 16, &k));
        ARROW_RETURN_NOT_OK(t_scratch.Get(kValidity, g + 16, &kv));
        ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2, g * 8 + 16, &s));
        ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2Validity, g * 8 + 16, &c));
        ARROW_RETURN_NOT_OK(t_scratch.Get(kOutValidity, g + 16, &nn));
        void *mn = nullptr, *mx = nullptr;
        if (needs_minmax_) {
          ARROW_RETURN_NOT_OK(t_scratch.Get(kOutData, g * 8 + 16, &mn));
          ARROW_RETURN_NOT_OK(t_scratch.Get(kBinWs, g * 8 + 16, &mx));
        }
        ARROW_RETURN_NOT_OK(FromArx(arx_groupby_export(state_, minmax_, (int32_t*)k, (uint8_t*)kv, (int64_t*)s,
                                                       (int64_t*)c, (uint8_t*)nn, (int64_t*)mn, (int64_t*)mx, st)));
        ARROW_RETURN_NOT_OK(FromArx(arx_groupby_sum_i64_merge(fresh, cap, (const int32_t*)k, (const uint8_t*)kv,
                                                              (const int64_t*)s, (const int64_t*)c,
                                                              (const uint8_t*)nn, g, st)));
        if (needs_minmax_) {
          ARROW_RETURN_NOT_OK(FromArx(arx_groupby_minmax_merge(fresh, fresh_minmax.ptr, cap, (const int32_t*)k,
                                                               (const uint8_t*)kv, (const int64_t*)mn,
                                                               (const int64_t*)mx, (const uint8_t*)nn, g, st)));
        }
      }
      HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
      // (the old table goes back to the pool when its buffers are replaced below)
    }
    state_buf_ = std::move(fresh_table.buffer);
    minmax_buf_ = std::move(fresh_minmax.buffer);
    state_ = fresh;
    minmax_ = fresh_minmax.ptr;
    capacity_ = cap;
    return Status::OK();
  }

  // The staging columns come from the plugin's device pool (size classes, reused by the next plan: a raw hipMalloc
  // of a GB-sized column costs tens to hundreds of ms) and double when they are full.
  Status GrowStaging(int64_t more) {
    if (staged_ + more <= staged_cap_) return Status::OK();
    const int64_t cap = std::max<int64_t>(2 * staged_cap_, std::max<int64_t>(staged_ + more, 1 << 22));
    ARROW_ASSIGN_OR_RAISE(auto nk, AllocDevice(cap * 4));
    ARROW_ASSIGN_OR_RAISE(auto nv, AllocDevice(cap * 8));
    if (staged_ > 0) {
      HIP_RETURN_NOT_OK(hipMemcpy(reinterpret_cast<void*>(nk->mutable_address()), d_keys_, staged_ * 4, hipMemcpyDeviceToDevice));
      HIP_RETURN_NOT_OK(hipMemcpy(reinterpret_cast<void*>(nv->mutable_address()), d_vals_, staged_ * 8, hipMemcpyDeviceToDevice));
    }
    keys_buf_ = std::move(nk);
    vals_buf_ = std::move(nv);
    d_keys_ = reinterpret_cast<void*>(keys_buf_->mutable_address());
    d_vals_ = reinterpret_cast<void*>(vals_buf_->mutable_address());
    staged_cap_ = cap;
    if (staged_valid_) ARROW_RETURN_NOT_OK(AllocStagedValidity(/*keep_rows=*/staged_));
    return Status::OK();
  }

  // (re)allocate the two staged validity bitmaps for staged_cap_ rows, zeroed behind the first keep_rows rows
  Status AllocStagedValidity(int64_t keep_rows) {
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    for (std::shared_ptr<Buffer>* buf : {&kvalid_buf_, &vvalid_buf_}) {
      ARROW_ASSIGN_OR_RAISE(auto fresh, AllocDevice(BitmapBytes(staged_cap_)));
      HIP_RETURN_NOT_OK(hipMemsetAsync(reinterpret_cast<void*>(fresh->mutable_address()), 0,
                                       static_cast<size_t>(BitmapBytes(staged_cap_)), st));
      if (keep_rows > 0 && *buf != nullptr) {
        HIP_RETURN_NOT_OK(hipMemcpyAsync(reinterpret_cast<void*>(fresh->mutable_address()),
                                         reinterpret_cast<const void*>((*buf)->address()),
                                         static_cast<size_t>((keep_rows + 7) / 8), hipMemcpyDeviceToDevice, st));
      }
      HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (the old bitmap goes back to the pool now)
      *buf = std::move(fresh);
    }
    return Status::OK();
  }

  // From now on the staged rows carry validity: the rows staged so far were all valid.
  Status EnableStagedValidity() {
    if (staged_valid_) return Status::OK();
    ARROW_RETURN_NOT_OK(AllocStagedValidity(0));
    staged_valid_ = true;
    if (staged_ > 0) ARROW_RETURN_NOT_OK(MarkStagedValid(0, staged_));
    return Status::OK();
  }

  // validity of staged rows [first, first + rows) = all ones, both columns (one launch)
  Status MarkStagedValid(int64_t first, int64_t rows) {
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    const ArxBitSeg segs[2] = {
        {nullptr, 0, reinterpret_cast<void*>(kvalid_buf_->mutable_address()), first, rows},
        {nullptr, 0, reinterpret_cast<void*>(vvalid_buf_->mutable_address()), first, rows}};
    void* d_segs = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(kFlag, sizeof(segs) + 64, &d_segs));
    HIP_RETURN_NOT_OK(hipMemcpyAsync(d_segs, segs, sizeof(segs), hipMemcpyHostToDevice, st));
    ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy_segments(static_cast<const ArxBitSeg*>(d_segs), 2, rows, st)));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (segs is a local)
    return Status::OK();
  }

  // The pending device batches -> the staging columns, one launch for all of them and both columns.
  Status FlushPending() {
    if (pending_.empty()) return Status::OK();
    ARROW_RETURN_NOT_OK(GrowStaging(pending_rows_));
    bool any_nulls = false;
    for (const PendingBatch& b : pending_) any_nulls = any_nulls || b.nulls;
    if (any_nulls) ARROW_RETURN_NOT_OK(EnableStagedValidity());
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    // the staging columns are pooled buffers that any Acero thread may have allocated: an error return between a launch
    // and its synchronisation must not hand them back to the pool while this thread's stream still writes them
    // (a RocmBuffer only waits for the stream of the thread that allocated it; ADVICE r2)
    struct SyncOnEarlyReturn {
      hipStream_t st;
      bool done = false;
      ~SyncOnEarlyReturn() {
        if (!done) (void)hipStreamSynchronize(st);
      }
    } guard{st};
    std::vector<ArxCopySeg> segs;
    std::vector<ArxBitSeg> bit_segs;   // the validity of the same rows, one more launch for all batches and both columns
    segs.reserve(2 * pending_.size());
    uint64_t longest = 0;
    int64_t longest_rows = 0;
    int64_t at = staged_;
    for (const PendingBatch& b : pending_) {
      const auto* ksrc = reinterpret_cast<const uint8_t*>(b.keys->buffers[1]->address()) + b.keys->offset * 4;
      const auto* vsrc = reinterpret_cast<const uint8_t*>(b.values->buffers[1]->address()) + b.values->offset * 8;
      segs.push_back(ArxCopySeg{ksrc, static_cast<int32_t*>(d_keys_) + at, static_cast<uint64_t>(b.rows) * 4});
      segs.push_back(ArxCopySeg{vsrc, static_cast<int64_t*>(d_vals_) + at, static_cast<uint64_t>(b.rows) * 8});
      longest = std::max<uint64_t>(longest, static_cast<uint64_t>(b.rows) * 8);
      if (staged_valid_) {
        auto bits_of = [](const ArrayData& a) -> const void* {   // (no bitmap, or a known zero null count: all ones)
          return a.buffers[0] != nullptr && a.null_count.load() != 0 ? reinterpret_cast<const void*>(a.buffers[0]->address())
                                                                     : nullptr;
        };
        bit_segs.push_back(ArxBitSeg{bits_of(*b.keys), b.keys->offset, reinterpret_cast<void*>(kvalid_buf_->mutable_address()), at, b.rows});
        bit_segs.push_back(ArxBitSeg{bits_of(*b.values), b.values->offset, reinterpret_cast<void*>(vvalid_buf_->mutable_address()), at, b.rows});
        longest_rows = std::max(longest_rows, b.rows);
      }
      at += b.rows;
    }
    void* d_segs = nullptr;
    const size_t seg_bytes = segs.size() * sizeof(ArxCopySeg), bit_bytes = bit_segs.size() * sizeof(ArxBitSeg);
    ARROW_RETURN_NOT_OK(t_scratch.Get(kFlag, seg_bytes + bit_bytes + 64, &d_segs));
    HIP_RETURN_NOT_OK(hipMemcpyAsync(d_segs, segs.data(), seg_bytes, hipMemcpyHostToDevice, st));
    ARROW_RETURN_NOT_OK(FromArx(arx_copy_segments(static_cast<const ArxCopySeg*>(d_segs), static_cast<int64_t>(segs.size()),
                                                  longest, st)));
    if (!bit_segs.empty()) {
      void* d_bits = static_cast<uint8_t*>(d_segs) + seg_bytes;
      HIP_RETURN_NOT_OK(hipMemcpyAsync(d_bits, bit_segs.data(), bit_bytes, hipMemcpyHostToDevice, st));
      ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy_segments(static_cast<const ArxBitSeg*>(d_bits),
                                                           static_cast<int64_t>(bit_segs.size()), longest_rows, st)));
    }
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // the batches' buffers may go now
    guard.done = true;
    staged_ = at;
    g_aggregate_flushes.fetch_add(1);
    pending_.clear();
    pending_rows_ = 0;
    return Status::OK();
  }

  // One device-resident batch into the state, where it lies (with the partitioned plans' workspace when it is large).
  Status ConsumeDevice(const ArrayData& k, const ArrayData& v, int64_t n, hipStream_t st) {
    PhaseTiming timing;
    ARROW_RETURN_NOT_OK(WidenKeyRange(reinterpret_cast<const void*>(k.buffers[1]->address()), k.offset, n, st));
    timing.Mark("key range");
    ARROW_RETURN_NOT_OK(EnsureState(staged_ + pending_rows_ + n));
    timing.Mark("table (alloc + init)");
    auto span_of = [](const ArrayData& a) {
      ArxSpan sp{};
      sp.validity = a.buffers[0] ? reinterpret_cast<const void*>(a.buffers[0]->address()) : nullptr;
      sp.data = reinterpret_cast<const void*>(a.buffers[1]->address());
      sp.offset = a.offset;
      sp.length = a.length;
      const int64_t nc = a.null_count.load();
      sp.null_count = sp.validity == nullptr ? 0 : (nc > 0 ? nc : (nc == 0 ? 0 : arrow::kUnknownNullCount));
      return sp;
    };
    ArxSpan dk = span_of(k), dv = span_of(v);
    const size_t ws_bytes = arx_groupby_consume_workspace_bytes(n, capacity_);
    void* ws = nullptr;
    if (ws_bytes > 0) {
      ARROW_RETURN_NOT_OK(t_scratch.Get(kWs, ws_bytes + 256, &ws));
      ws = Align256(ws);
    }
    ARROW_RETURN_NOT_OK(FromArx(arx_groupby_sum_i64_consume(state_, capacity_, &dk, &dv, ws, ws_bytes, st)));
    if (needs_minmax_) {
      ARROW_RETURN_NOT_OK(FromArx(arx_groupby_minmax_i64_consume(state_, minmax_, capacity_, &dk, &dv, st)));
    }
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    timing.Mark("consume (direct)");
    rows_seen_ += n;
    CountGpu(kFnHashSum);
    return Status::OK();
  }

  // the run of consecutive device slices gathered by Consume: one ConsumeDevice over all of it
  Status FlushSpan(hipStream_t st) {
    if (span_rows_ == 0) return Status::OK();
    auto whole = [&](const ArrayData& first) {
      auto merged = first.Copy();
      merged->length = span_rows_;
      merged->null_count = (first.buffers[0] == nullptr || !span_nulls_) ? 0 : arrow::kUnknownNullCount;
      return merged;
    };
    const auto k = whole(*span_k_), v = whole(*span_v_);
    const int64_t n = span_rows_;
    span_rows_ = 0;
    span_k_.reset();
    span_v_.reset();
    return ConsumeDevice(*k, *v, n, st);
  }

  Status Consume(const cp::ExecBatch& batch) {
    const int64_t n = batch.length;
    if (n == 0) return Status::OK();
    if (!batch[key_idx_].is_array() || !batch[val_idx_].is_array()) {
      return Status::NotImplemented("aggregate_rocm: scalar columns");
    }
    const ArrayData& k = *batch[key_idx_].array();
    const ArrayData& v = *batch[val_idx_].array();
    // device-resident batches (kROCM buffers): no staging over PCIe, and never a CPU popcount —
    // a sliced device array with an unknown null count is treated as "may have nulls"
    const bool on_device = DataOnRocm(k) || DataOnRocm(v);
    if (on_device && !(DataOnRocm(k) && DataOnRocm(v))) {
      return Status::Invalid("aggregate_rocm: key and value columns must both be host or both be device arrays");
    }
    saw_device_rows_ = saw_device_rows_ || on_device;
    const bool nulls = on_device ? (k.buffers[0] != nullptr && k.null_count.load() != 0) ||
                                       (v.buffers[0] != nullptr && v.null_count.load() != 0)
                                 : (k.GetNullCount() != 0) || (v.GetNullCount() != 0);
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    if (on_device && n >= g_aggregate_direct_rows.load()) {
      // a large device batch (table_source_rocm's, or a big chunk from any source): one partitioned pass over the batch
      // where it lies — staging exists to gather 32K-row morsels, and costs a copy of every row.  Batches that are
      // CONSECUTIVE SLICES of the same buffers (what a source cuts one device column into) are one span: the pass runs once
      // over all of them when the run ends — every pass flushes every group and pays the key-range read-back, and 30
      // passes over 2^27 rows took 80 ms where one pass over the 4e9 rows takes 43 (profiles/r05_i_*)
      g_aggregate_direct_batches.fetch_add(1);
      auto continues = [](const ArrayData& prev, int64_t prev_rows, const ArrayData& next) {
        if (prev.buffers.size() != next.buffers.size() || prev.offset + prev_rows != next.offset) return false;
        for (size_t j = 0; j < prev.buffers.size(); ++j) {
          if (prev.buffers[j] != next.buffers[j]) return false;
        }
        return true;
      };
      if (span_rows_ > 0 && continues(*span_k_, span_rows_, k) && continues(*span_v_, span_rows_, v)) {
        span_rows_ += n;
        span_nulls_ = span_nulls_ || nulls;
        return Status::OK();
      }
      ARROW_RETURN_NOT_OK(FlushSpan(st));
      span_k_ = batch[key_idx_].array();
      span_v_ = batch[val_idx_].array();
      span_rows_ = n;
      span_nulls_ = nulls;
      return Status::OK();
    }
    // (ADVICE r5: a span in progress is consumed before any batch takes another route — its errors surface with the batch
    //  that ended it, and nothing about the span is left implicit; sums and extrema commute, so the result is the same)
    ARROW_RETURN_NOT_OK(FlushSpan(st));
    if (on_device && (!nulls || g_aggregate_stage_nulls.load())) {
      // device-resident batch without nulls: remember it (the buffers stay alive with the batch's ArrayData) and copy
      // the pending batches into the staging columns 2M rows at a time with ONE launch (arx_copy_segments) — a copy
      // per 32K-row morsel and column is what bounded these plans
      pending_.push_back(PendingBatch{batch[key_idx_].array(), batch[val_idx_].array(), n, nulls});
      pending_rows_ += n;
      if (pending_rows_ >= g_aggregate_flush_rows.load()) ARROW_RETURN_NOT_OK(FlushPending());
      return Status::OK();
    }
    if (!nulls) {
      ARROW_RETURN_NOT_OK(FlushPending());   // keep the staged rows in arrival order (not needed for sums; cheap)
      // append to the device staging buffers; consumed in one partitioned pass at the end
      ARROW_RETURN_NOT_OK(GrowStaging(n));
      const void* ksrc = on_device ? reinterpret_cast<const void*>(k.buffers[1]->address() + k.offset * 4)
                                   : static_cast<const void*>(k.GetValues<int32_t>(1));
      const void* vsrc = on_device ? reinterpret_cast<const void*>(v.buffers[1]->address() + v.offset * 8)
                                   : static_cast<const void*>(v.GetValues<int64_t>(1));
      const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
      HIP_RETURN_NOT_OK(hipMemcpy(static_cast<int32_t*>(d_keys_) + staged_, ksrc, n * 4, kind));
      HIP_RETURN_NOT_OK(hipMemcpy(static_cast<int64_t*>(d_vals_) + staged_, vsrc, n * 8, kind));
      if (staged_valid_) ARROW_RETURN_NOT_OK(MarkStagedValid(staged_, n));
      staged_ += n;
      return Status::OK();
    }
    if (on_device) return ConsumeDevice(k, v, n, st);
    key_range_complete_ = false;   // (host rows with nulls are consumed as they come: their keys' range is not looked at)
    ARROW_RETURN_NOT_OK(EnsureState(staged_ + pending_rows_ + n));
    ArxSpan dk{}, dv{};
    ARROW_RETURN_NOT_OK(Upload(ArraySpan(k), 4, kValues, kValidity, st, &dk));
    ARROW_RETURN_NOT_OK(Upload(ArraySpan(v), 8, kArg2, kArg2Validity, st, &dv));
    ARROW_RETURN_NOT_OK(FromArx(arx_groupby_sum_i64_consume(state_, capacity_, &dk, &dv, nullptr, 0, st)));
    if (needs_minmax_) {
      ARROW_RETURN_NOT_OK(FromArx(arx_groupby_minmax_i64_consume(state_, minmax_, capacity_, &dk, &dv, st)));
    }
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    rows_seen_ += n;
    CountGpu(kFnHashSum);
    return Status::OK();
  }

  // ARROW_AMD_AGGREGATE_TIMING=1: wall ms of the phases of Finish on stderr (diagnostics for the bench's Acero leg)
  struct PhaseTiming {
    bool on = std::getenv("ARROW_AMD_AGGREGATE_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void Mark(const char* what) {
      if (!on) return;
      const auto t1 = std::chrono::steady_clock::now();
      std::fprintf(stderr, "[aggregate_rocm] %-22s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
      t0 = t1;
    }
  };

  // The whole input was ONE run of device slices without nulls and only sums / counts are asked for: the rows go through
  // the RANGE-PARTITIONED state (include/arrow_amd.h arx_groupby_range_*; csrc/groupby_lines.h) — a sampled key range
  // instead of WidenKeyRange's pass over every key, no table to allocate, insert into and export.  *done == false (and
  // nothing consumed, the span untouched) when the keys do not suit the state: a wide or tiny range, a key the sample
  // missed, a hot key; Finish goes on with the table then.  On success k / s / c / ones hold what arx_groupby_export
  // would have produced (`ones`: every key valid, no group saw a null), ascending by key.
  Status TryRangeState(hipStream_t st, PhaseTiming* timing, bool* done, int64_t* num_groups, void** k, void** s, void** c,
                       void** ones) {
    *done = false;
    auto whole = [&](const ArrayData& first) {
      ArxSpan sp{};
      sp.validity = nullptr;
      sp.data = reinterpret_cast<const void*>(first.buffers[1]->address());
      sp.offset = first.offset;
      sp.length = span_rows_;
      sp.null_count = 0;
      return sp;
    };
    ArxSpan dk = whole(*span_k_), dv = whole(*span_v_);
    void* pair = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(kFlag, 64, &pair));
    const int32_t init[2] = {std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()};
    HIP_RETURN_NOT_OK(hipMemcpyAsync(pair, init, 8, hipMemcpyHostToDevice, st));
    ARROW_RETURN_NOT_OK(FromArx(arx_groupby_key_range_sampled_i32(&dk, g_aggregate_range_sample_rows.load(),
                                                                  static_cast<int32_t*>(pair), st)));
    int32_t mm[2];
    HIP_RETURN_NOT_OK(hipMemcpyAsync(mm, pair, 8, hipMemcpyDeviceToHost, st));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    timing->Mark("key range (sampled)");
    if (mm[0] > mm[1]) return Status::OK();
    // (the sample misses a few keys at both ends: 1/64 of the range on each side, as the mirror's RangeGroupBySum.plan_for)
    const int64_t pad = (int64_t(mm[1]) - mm[0] + 1) / 64 + 1;
    const int32_t lo = static_cast<int32_t>(std::max<int64_t>(std::numeric_limits<int32_t>::min(), int64_t(mm[0]) - pad));
    const int32_t hi = static_cast<int32_t>(std::min<int64_t>(std::numeric_limits<int32_t>::max(), int64_t(mm[1]) + pad));
    ArxRangePlan plan{};
    const int rc_plan = arx_groupby_range_plan(span_rows_, lo, hi, &plan);
    if (rc_plan == ARX_NOT_IMPLEMENTED) return Status::OK();
    ARROW_RETURN_NOT_OK(FromArx(rc_plan));
    ARROW_ASSIGN_OR_RAISE(std::shared_ptr<Buffer> state, AllocDevice(plan.state_bytes));
    void* blocks = reinterpret_cast<void*>(state->mutable_address());
    HIP_RETURN_NOT_OK(hipMemsetAsync(blocks, 0, static_cast<size_t>(plan.state_bytes), st));
    void* ws = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(kWs, static_cast<size_t>(plan.workspace_bytes) + 256, &ws));
    ws = Align256(ws);
    const int rc = arx_groupby_range_sum_i64_consume(blocks, &plan, &dk, &dv, ws, static_cast<size_t>(plan.workspace_bytes), st);
    if (rc == ARX_CAPACITY_ERROR || rc == ARX_NOT_IMPLEMENTED) {
      g_aggregate_range_declined.fetch_add(1);
      timing->Mark("range state (declined)");
      return Status::OK();
    }
    ARROW_RETURN_NOT_OK(FromArx(rc));
    timing->Mark("consume (range state)");
    const int64_t slots = plan.slots;
    void *fws = nullptr, *count = nullptr;
    const size_t fws_bytes = arx_groupby_range_finalize_workspace_bytes(slots);
    ARROW_RETURN_NOT_OK(t_scratch.Get(kValues, slots * 4 + 16, k));
    ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2, slots * 8 + 16, s));
    ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2Validity, slots * 8 + 16, c));
    ARROW_RETURN_NOT_OK(t_scratch.Get(kValidity, slots + 16, ones));
    ARROW_RETURN_NOT_OK(t_scratch.Get(kBinWs, fws_bytes + 256, &fws));
    fws = Align256(fws);
    ARROW_RETURN_NOT_OK(t_scratch.Get(kCounter, 64, &count));
    HIP_RETURN_NOT_OK(hipMemsetAsync(count, 0, 8, st));
    ARROW_RETURN_NOT_OK(FromArx(arx_groupby_range_finalize(blocks, plan.key_min, plan.width, plan.partitions, 0, fws, fws_bytes,
                                                           static_cast<int32_t*>(*k), static_cast<int64_t*>(*s),
                                                           static_cast<int64_t*>(*c), static_cast<uint8_t*>(*ones),
                                                           static_cast<int64_t*>(count), st)));
    HIP_RETURN_NOT_OK(hipMemcpyAsync(num_groups, count, 8, hipMemcpyDeviceToHost, st));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    timing->Mark("finalize (range state)");
    rows_seen_ += span_rows_;
    span_rows_ = 0;
    span_k_.reset();
    span_v_.reset();
    g_aggregate_range_plans.fetch_add(1);
    CountGpu(kFnHashSum);
    *done = true;
    return Status::OK();
  }

  Status Finish() override {
    PhaseTiming timing;
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    bool range_done = false;
    int64_t g = 0;
    void *k = nullptr, *kv = nullptr, *s = nullptr, *c = nullptr, *nn = nullptr;
    if (g_aggregate_range_state.load() && span_rows_ >= g_aggregate_range_min_rows.load() && rows_seen_ == 0 && staged_ == 0 &&
        pending_.empty() && !span_nulls_ && !needs_minmax_ && state_ == nullptr) {
      void* ones = nullptr;
      ARROW_RETURN_NOT_OK(TryRangeState(st, &timing, &range_done, &g, &k, &s, &c, &ones));
      kv = nn = ones;
    }
    if (range_done) return FinishColumns(st, &timing, true, g, k, kv, s, c, nn);
    ARROW_RETURN_NOT_OK(FlushSpan(st));
    ARROW_RETURN_NOT_OK(FlushPending());
    timing.Mark("flush pending");
    if (staged_ > 0) ARROW_RETURN_NOT_OK(WidenKeyRange(d_keys_, 0, staged_, st));
    ARROW_RETURN_NOT_OK(EnsureState(staged_));
    if (staged_ > 0) {
      ArxSpan dk{nullptr, d_keys_, 0, staged_, 0}, dv{nullptr, d_vals_, 0, staged_, 0};
      if (staged_valid_) {
        dk.validity = reinterpret_cast<const void*>(kvalid_buf_->address());
        dv.validity = reinterpret_cast<const void*>(vvalid_buf_->address());
        dk.null_count = dv.null_count = arrow::kUnknownNullCount;
      }
      const size_t ws_bytes = arx_groupby_consume_workspace_bytes(staged_, capacity_);
      void* ws = nullptr;
      if (ws_bytes > 0) {
        ARROW_RETURN_NOT_OK(t_scratch.Get(kWs, ws_bytes + 256, &ws));
        ws = Align256(ws);
      }
      ARROW_RETURN_NOT_OK(FromArx(arx_groupby_sum_i64_consume(state_, capacity_, &dk, &dv, ws, ws_bytes, st)));
      if (needs_minmax_) {
        ARROW_RETURN_NOT_OK(FromArx(arx_groupby_minmax_i64_consume(state_, minmax_, capacity_, &dk, &dv, st)));
      }
      rows_seen_ += staged_;
      staged_ = 0;
      CountGpu(kFnHashSum);
    }
    ARROW_RETURN_NOT_OK(FromArx(arx_groupby_num_groups(state_, &g, st)));
    timing.Mark("consume staged rows");
    return FinishColumns(st, &timing, false, g, k, kv, s, c, nn);
  }

  // The result columns of g groups: from the table (arx_groupby_export) or, exported == true, from the arrays the range
  // state's finalize already wrote.
  Status FinishColumns(hipStream_t st, PhaseTiming* timing_in, bool exported, int64_t g, void* k, void* kv, void* s, void* c,
                       void* nn) {
    PhaseTiming& timing = *timing_in;
    void* ok = nullptr;
    arrow::MemoryPool* pool = plan_->query_context()->memory_pool();
    auto mark_alloc = [&]() { timing.Mark("  buffers + scratch"); };
    // Results leave the device in bulk: large columns into pooled page-locked host buffers (AllocateResultBuffer),
    // validity packed to bitmaps ON the device (arx_bytes_to_bitmap) with its count — 10M groups were 19 ms of pageable
    // copies and a CPU BytesToBits per column before, against 6 ms for the aggregation itself.
    // aggregate_device_output: a plan whose rows arrived in HBM may keep its result there as well (kROCM arrays with
    // exact null counts; nothing crosses PCIe) — off by default, the reference's node produces host arrays.
    const bool device_out = g_aggregate_device_output.load() && saw_device_rows_;
    auto result_buffer = [&](int64_t bytes) -> arrow::Result<std::shared_ptr<Buffer>> {
      if (device_out) return AllocDevice(std::max<int64_t>(bytes, 8));
      return AllocateResultBuffer(bytes, pool);
    };
    auto out_ptr = [&](const std::shared_ptr<Buffer>& b) -> void* {
      if (device_out) return reinterpret_cast<void*>(b->mutable_address());
      return b->mutable_data();
    };
    const hipMemcpyKind out_kind = device_out ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    // Column-sized copies are done by a KERNEL (arx_buffer_copy), not by hipMemcpyAsync: the copy engines move
    // device-to-device at ~30 GB/s and device-to-pinned-host at ~18 GB/s here, a kernel writes HBM at 6 TB/s and
    // page-locked host memory (mapped into the device's address space) at the link's rate.
    auto copy_out = [&](const std::shared_ptr<Buffer>& dst, const void* src, int64_t bytes) -> Status {
      const bool mapped = device_out || dynamic_cast<const PinnedHostBuffer*>(dst.get()) != nullptr;   // (a kernel cannot write pageable host memory)
      if (mapped && g_results_kernel_copy.load()) {
        return FromArx(arx_buffer_copy(src, out_ptr(dst), bytes, st));
      }
      HIP_RETURN_NOT_OK(hipMemcpyAsync(out_ptr(dst), src, static_cast<size_t>(bytes), out_kind, st));
      return Status::OK();
    };
    ARROW_ASSIGN_OR_RAISE(std::shared_ptr<Buffer> keys, result_buffer(g * 4));
    std::vector<arrow::Datum> columns(1 + aggs_.size());
    void *mn = nullptr, *mx = nullptr;
    void *d_bits = nullptr, *d_count = nullptr;
    const int64_t bitmap_bytes = arrow::bit_util::BytesForBits(g);
    if (g > 0) {
      if (!exported) {
        ARROW_RETURN_NOT_OK(t_scratch.Get(kValues, g * 4 + 16, &k));
        ARROW_RETURN_NOT_OK(t_scratch.Get(kValidity, g + 16, &kv));
        ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2, g * 8 + 16, &s));
        ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2Validity, g * 8 + 16, &c));
        ARROW_RETURN_NOT_OK(t_scratch.Get(kOutValidity, g + 16, &nn));
      }
      ARROW_RETURN_NOT_OK(t_scratch.Get(kOutData, g + 16, &ok));
      ARROW_RETURN_NOT_OK(t_scratch.Get(kWs, static_cast<size_t>((g + 63) / 64 * 8 + 64), &d_bits));   // (the consume's workspace is done with)
      d_count = static_cast<uint8_t*>(d_bits) + (g + 63) / 64 * 8 + 32;
      if (needs_minmax_) {
        ARROW_RETURN_NOT_OK(t_scratch.Get(kBinWs, g * 16 + 32, &mn));
        mx = static_cast<uint8_t*>(mn) + ((g * 8 + 15) & ~int64_t(15));
      }
      mark_alloc();
      if (!exported) {
        ARROW_RETURN_NOT_OK(FromArx(arx_groupby_export(state_, minmax_, (int32_t*)k, (uint8_t*)kv, (int64_t*)s,
                                                       (int64_t*)c, (uint8_t*)nn, (int64_t*)mn, (int64_t*)mx, st)));
      }
      if (timing.on) {
        HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
        timing.Mark("  export kernel");
      }
      ARROW_RETURN_NOT_OK(copy_out(keys, k, g * 4));
      if (timing.on) {
        HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
        timing.Mark("  keys copied out");
      }
    }
    // one byte per group on the device -> (bitmap or none, null count) on the host; synchronises the stream
    auto pack_validity = [&](const void* bytes, std::shared_ptr<Buffer>* bits, int64_t* null_count) -> Status {
      *bits = nullptr;
      *null_count = 0;
      if (g == 0) return Status::OK();
      HIP_RETURN_NOT_OK(hipMemsetAsync(d_count, 0, 8, st));
      ARROW_RETURN_NOT_OK(FromArx(arx_bytes_to_bitmap(static_cast<const uint8_t*>(bytes), g, d_bits,
                                                      static_cast<int64_t*>(d_count), st)));
      int64_t valid = 0;
      HIP_RETURN_NOT_OK(hipMemcpyAsync(&valid, d_count, 8, hipMemcpyDeviceToHost, st));
      HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
      *null_count = g - valid;
      if (*null_count == 0) return Status::OK();   // (the reference allocates a bitmap only when a group is null)
      ARROW_ASSIGN_OR_RAISE(*bits, result_buffer(bitmap_bytes));
      ARROW_RETURN_NOT_OK(copy_out(*bits, d_bits, bitmap_bytes));
      HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
      return Status::OK();
    };
    for (size_t ai = 0; ai < aggs_.size(); ++ai) {
      const AggSpec& spec = aggs_[ai];
      ARROW_ASSIGN_OR_RAISE(std::shared_ptr<Buffer> data, result_buffer(g * 8));
      std::shared_ptr<Buffer> bits;
      int64_t null_count = 0;
      if (spec.kind == kCount) {
        // GroupedCountImpl (hash_aggregate.cc): the count of valid values, never null
        if (g > 0) ARROW_RETURN_NOT_OK(copy_out(data, c, g * 8));
        HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
      } else if (spec.kind == kMin || spec.kind == kMax) {
        // GroupedMinMaxImpl::Finalize (hash_aggregate.cc:401-419): null where the group saw no value
        // (or, with !skip_nulls, saw a null); the reference writes the anti-extremum there, we write 0
        // only into the validity — the data slot keeps the anti-extremum as well
        if (g > 0) {
          ARROW_RETURN_NOT_OK(FromArx(arx_groupby_minmax_finalize((const int64_t*)mn, (const int64_t*)mx,
                                                                  (const uint8_t*)nn, g,
                                                                  spec.options.skip_nulls ? 1 : 0, (uint8_t*)ok, st)));
          ARROW_RETURN_NOT_OK(copy_out(data, spec.kind == kMin ? mn : mx, g * 8));
        }
        ARROW_RETURN_NOT_OK(pack_validity(ok, &bits, &null_count));
      } else if (spec.kind == kMean) {
        // GroupedMeanImpl (hash_aggregate_numeric.cc:352-430): doubles summed in row order == (double)sum / count while
        // every partial sum is an exact integer; arx_groupby_mean_i64_finalize checks the bound per group
        uint32_t inexact = 0;
        if (g > 0) {
          void* flag = nullptr;
          ARROW_RETURN_NOT_OK(t_scratch.Get(kFlag, 64, &flag));
          HIP_RETURN_NOT_OK(hipMemsetAsync(flag, 0, 4, st));
          void* dmeans = nullptr;
          ARROW_RETURN_NOT_OK(t_scratch.Get(kCounter, g * 8 + 16, &dmeans));
          ARROW_RETURN_NOT_OK(FromArx(arx_groupby_mean_i64_finalize((const int64_t*)s, (const int64_t*)c, (const int64_t*)mn,
                                                                    (const int64_t*)mx, (const uint8_t*)nn, g,
                                                                    spec.options.skip_nulls ? 1 : 0, spec.options.min_count,
                                                                    (double*)dmeans, (uint8_t*)ok, (uint32_t*)flag, st)));
          ARROW_RETURN_NOT_OK(copy_out(data, dmeans, g * 8));
          HIP_RETURN_NOT_OK(hipMemcpyAsync(&inexact, flag, 4, hipMemcpyDeviceToHost, st));
        }
        ARROW_RETURN_NOT_OK(pack_validity(ok, &bits, &null_count));
        if (inexact != 0) {
          return Status::NotImplemented("aggregate_rocm: hash_mean(int64): a group's partial sums exceed 2^53, where the "
                                        "reference's row-order double accumulation depends on the row order");
        }
      } else {
        if (g > 0) {
          ARROW_RETURN_NOT_OK(FromArx(arx_groupby_sum_i64_finalize((const int64_t*)c, (const uint8_t*)nn, g,
                                                                   spec.options.skip_nulls ? 1 : 0,
                                                                   spec.options.min_count, (uint8_t*)ok, st)));
          ARROW_RETURN_NOT_OK(copy_out(data, s, g * 8));
        }
        ARROW_RETURN_NOT_OK(pack_validity(ok, &bits, &null_count));   // (synchronises: `ok` is reused by the next aggregate)
      }
      std::vector<std::shared_ptr<Buffer>> bufs{std::move(bits), std::move(data)};
      columns[1 + ai] = arrow::Datum(ArrayData::Make(spec.kind == kMean ? arrow::float64() : arrow::int64(), g, std::move(bufs), null_count));
    }
    timing.Mark("  aggregate columns");
    std::shared_ptr<Buffer> kbits;
    int64_t key_nulls = 0;
    ARROW_RETURN_NOT_OK(pack_validity(kv, &kbits, &key_nulls));   // (at most the one group of the null key)
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    std::vector<std::shared_ptr<Buffer>> kbufs{std::move(kbits), std::move(keys)};
    columns[0] = arrow::Datum(ArrayData::Make(arrow::int32(), g, std::move(kbufs), key_nulls));
    // GroupByNode hands its result on in batches of ExecPlan::kMaxBatchSize rows (groupby_aggregate_node.cc OutputResult);
    // so does this node — unless the plan fed it larger batches (table_source_rocm), in which case every node in it
    // takes batches of that size and the result goes on at the same granularity (10M groups: 1 batch instead of 306)
    const int64_t batch_size = std::max<int64_t>(ac::ExecPlan::kMaxBatchSize, largest_input_batch_);
    timing.Mark("results to host");
    ARROW_RETURN_NOT_OK(EmitResult(this, output_, std::move(columns), g, device_out, st, batch_size));
    timing.Mark("batches handed on");
    return Status::OK();
  }

  const int key_idx_, val_idx_;
  const std::vector<AggSpec> aggs_;
  bool needs_minmax_ = false;
  void* minmax_ = nullptr;   // mins | maxes per slot (arx_groupby_minmax_bytes), only with hash_min / hash_max
  void* state_ = nullptr;
  int64_t capacity_ = 0;
  std::shared_ptr<Buffer> keys_buf_, vals_buf_;   // the staging columns (pooled device buffers)
  std::shared_ptr<Buffer> state_buf_, minmax_buf_; // the table (pooled device buffers; state_ / minmax_ point into them)
  void* d_keys_ = nullptr;
  void* d_vals_ = nullptr;
  int64_t staged_ = 0, staged_cap_ = 0, rows_seen_ = 0;
  // validity of the staged rows (keys, values): kept only once a batch with nulls has been staged (staged_valid_);
  // bits of the rows behind staged_ are zero, which is what arx_bitmap_copy_segments ORs into
  std::shared_ptr<Buffer> kvalid_buf_, vvalid_buf_;
  bool staged_valid_ = false;
  struct PendingBatch {
    std::shared_ptr<ArrayData> keys, values;
    int64_t rows;
    bool nulls;
  };
  int64_t largest_input_batch_ = 0;
  bool saw_device_rows_ = false;
  std::shared_ptr<ArrayData> span_k_, span_v_;   // the first of a run of consecutive large device slices (its buffers = the run's)
  int64_t span_rows_ = 0;
  bool span_nulls_ = false;
  std::vector<PendingBatch> pending_;   // device batches not yet copied into the staging columns
  int32_t key_lo_ = INT32_MAX, key_hi_ = INT32_MIN;   // range of the keys consumed or about to be (WidenKeyRange); empty: unknown
  bool key_range_complete_ = true;     // false once rows were consumed without their keys' range (host batches)
  int64_t pending_rows_ = 0;
};

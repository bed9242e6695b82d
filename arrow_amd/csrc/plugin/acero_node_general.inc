// aggregate_rocm for everything the fused int32 -> int64 operator does not take: the device Grouper + dense hash kernels.
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- Acero: general device group-by node
// GroupByNode's own structure (acero/groupby_aggregate_node.cc:210-337: Grouper::Consume -> dense ids -> one
// HashAggregateKernel per aggregate -> GetUniques ++ Finalize) with every step on the device:
//   keys        1-32 fixed-width columns of 1 / 2 / 4 / 8 bytes (row/grouper.cc:559-611's fixed-width classes): int64 /
//               uint64 keys over their whole range, (int32, int32), (date32, int16, uint8) ...; rows of more than 16
//               bytes or 8 columns go through a chain of Grouper tables (see Finish)
//   aggregates  hash_sum / hash_mean / hash_min / hash_max over int64 columns (each its own column), hash_count (the
//               three CountOptions modes) over any fixed-width column, hash_count_all, hash_any / hash_all over boolean
//               columns (three dense counts per group, as plugin/hash_aggregate_bool.inc keeps them)
// The batches are kept until the input ends (AccumulatingNode, plugin/acero_common.inc), their columns
// concatenated into device staging columns — device-resident batches by ONE segment-copy launch per column, host batches
// by arrow::Concatenate + one upload — then ONE Grouper consume and one dense consume per aggregate run over all rows.
// Output = key columns ++ aggregate columns, groups in order of first appearance.
class RocmGroupByGeneralNode : public AccumulatingNode {
 public:
  enum Kind { kSum, kMean, kMin, kMax, kCount, kCountAll, kAny, kAll, kCountDistinct, kFirst, kLast, kOne, kProduct, kFirstLast, kList, kDistinct,
              kVariance, kStddev, kSkew, kKurtosis };
  struct Agg {
    Kind kind = kSum;
    int col = -1;                        // input column (-1: hash_count_all)
    cp::ScalarAggregateOptions options;
    int count_mode = ARX_COUNT_ONLY_VALID;
    int num_type = ARX_NUM_INT64;        // sum / mean / min / max: the value column's integer type (narrow ones are widened on the device)
    std::shared_ptr<arrow::DataType> out_type;   // the type of the column this aggregate computes
    int pair = 0;                        // hash_min_max = a hash_min (pair 1) and a hash_max (pair 2) that leave as ONE struct column
    int ddof = 0;                        // hash_variance / hash_stddev (VarianceOptions)
    bool biased = true;                  // hash_skew / hash_kurtosis (SkewOptions)
  };

  RocmGroupByGeneralNode(ac::ExecPlan* plan, std::vector<ac::ExecNode*> inputs, std::shared_ptr<arrow::Schema> out_schema,
                         std::vector<int> key_cols, std::vector<int> key_widths, std::vector<Agg> aggs)
      : AccumulatingNode(plan, std::move(inputs), {"input"}, std::move(out_schema)), key_cols_(std::move(key_cols)),
        key_widths_(std::move(key_widths)), aggs_(std::move(aggs)) {}

  // nullptr result = "not this node's case" is expressed as NotImplemented with the reason
  static arrow::Result<ac::ExecNode*> Make(ac::ExecPlan* plan, std::vector<ac::ExecNode*> inputs,
                                           const ac::AggregateNodeOptions& opts) {
    const auto& in_schema = *inputs[0]->output_schema();
    if (opts.keys.empty() || opts.keys.size() > 32 || !opts.segment_keys.empty() || opts.aggregates.empty()) {
      return Status::NotImplemented("aggregate_rocm: 1 to 32 keys, no segment keys, at least one aggregate");
    }
    std::vector<int> key_cols, key_widths;
    std::vector<std::shared_ptr<arrow::Field>> fields;
    for (const auto& ref : opts.keys) {
      ARROW_ASSIGN_OR_RAISE(auto path, ref.FindOne(in_schema));
      if (path.indices().size() != 1) return Status::NotImplemented("aggregate_rocm: nested field references");
      const auto& f = in_schema.field(path[0]);
      const int w = IsInt32Binary(*f->type()) ? 0 : FixedByteWidth(*f->type());   // 0: a utf8 / binary key (see Finish)
      if (!(w == 0 && IsInt32Binary(*f->type())) && w != 1 && w != 2 && w != 4 && w != 8) {
        return Status::NotImplemented("aggregate_rocm: key column ", f->name(), " of type ", f->type()->ToString(),
                                      " (fixed-width keys of 1, 2, 4 or 8 bytes, utf8 / binary keys)");
      }
      key_cols.push_back(path[0]);
      key_widths.push_back(w);
      fields.push_back(f);
    }
    std::vector<Agg> aggs;
    for (const auto& agg : opts.aggregates) {
      Agg spec;
      const std::string& fn = agg.function;
      if (fn == "hash_count_all") {
        spec.kind = kCountAll;
        spec.out_type = arrow::int64();
        aggs.push_back(spec);
        fields.push_back(arrow::field(agg.name, arrow::int64()));
        continue;
      }
      if (agg.target.size() != 1) return Status::NotImplemented("aggregate_rocm: unary aggregates only");
      ARROW_ASSIGN_OR_RAISE(auto vpath, agg.target[0].FindOne(in_schema));
      if (vpath.indices().size() != 1) return Status::NotImplemented("aggregate_rocm: nested field references");
      spec.col = vpath[0];
      const auto& vtype = *in_schema.field(spec.col)->type();
      if (fn == "hash_count_distinct") {
        // GroupedCountDistinctImpl (kernels/hash_aggregate.cc:1400-1478): a Grouper over (value, group id) pairs, the distinct
        // pairs counted per group — here the device Grouper over the staged value column and the rows' group ids
        spec.kind = kCountDistinct;
        const int w = FixedByteWidth(vtype);
        if (w == 0 || w > 8) {
          return Status::NotImplemented("aggregate_rocm: hash_count_distinct of ", vtype.ToString(), " columns (fixed-width values of up to 8 bytes)");
        }
        if (agg.options != nullptr) {
          const auto* co = dynamic_cast<const cp::CountOptions*>(agg.options.get());
          if (co == nullptr) return Status::TypeError("aggregate_rocm: hash_count_distinct takes CountOptions");
          spec.count_mode = co->mode == cp::CountOptions::ONLY_VALID ? ARX_COUNT_ONLY_VALID
                            : co->mode == cp::CountOptions::ONLY_NULL ? ARX_COUNT_ONLY_NULL : ARX_COUNT_ALL;
        }
        fields.push_back(arrow::field(agg.name, arrow::int64()));
        spec.out_type = arrow::int64();
        aggs.push_back(spec);
        continue;
      }
      if (fn == "hash_count") {
        spec.kind = kCount;
        if (FixedByteWidth(vtype) == 0 && vtype.id() != Type::BOOL) {
          return Status::NotImplemented("aggregate_rocm: hash_count of ", vtype.ToString(), " columns");
        }
        if (agg.options != nullptr) {
          const auto* co = dynamic_cast<const cp::CountOptions*>(agg.options.get());
          if (co == nullptr) return Status::TypeError("aggregate_rocm: hash_count takes CountOptions");
          spec.count_mode = co->mode == cp::CountOptions::ONLY_VALID ? ARX_COUNT_ONLY_VALID
                            : co->mode == cp::CountOptions::ONLY_NULL ? ARX_COUNT_ONLY_NULL : ARX_COUNT_ALL;
        }
        fields.push_back(arrow::field(agg.name, arrow::int64()));
      } else if (fn == "hash_sum" || fn == "hash_mean" || fn == "hash_min" || fn == "hash_max" || fn == "hash_min_max") {
        // hash_min_max (GroupedMinMaxImpl's own output, kernels/hash_aggregate.cc:330-419): struct<min, max> — computed as a
        // hash_min and a hash_max over the column, joined when the columns leave
        spec.kind = fn == "hash_sum" ? kSum : fn == "hash_mean" ? kMean : fn == "hash_max" ? kMax : kMin;
        spec.pair = fn == "hash_min_max" ? 1 : 0;
        // every integer width (hash_sum: int64 / uint64 output as the reference's accumulator types; the extrema of uint64
        // on x + 2^63 read as int64, the order-preserving map) — plugin/hash_aggregate.inc WidenTo64 / FlipUInt64
        // round 4: hash_min / hash_max also of float32 / float64 (order keys) and the temporal types (their int32 / int64)
        spec.num_type = (spec.kind == kMin || spec.kind == kMax) ? MinMaxNumType(vtype.id()) : SumNumType(vtype.id());
        // decimal128: hash_sum / hash_mean (128-bit sums; the mean's rounding division on the host) and hash_min / hash_max
        // (sorted runs, csrc/decimal.hip)
        if (vtype.id() == Type::DECIMAL128) spec.num_type = kNumDec128;
        if (spec.num_type < 0) {
          return Status::NotImplemented("aggregate_rocm: ", fn, " of ", vtype.ToString(), " columns (",
                                        (spec.kind == kMin || spec.kind == kMax) ? "integer, floating-point or temporal" : "integer or floating-point",
                                        " values)");
        }
        if (agg.options != nullptr) {
          const auto* so = dynamic_cast<const cp::ScalarAggregateOptions*>(agg.options.get());
          if (so == nullptr) return Status::TypeError("aggregate_rocm: ", fn, " takes ScalarAggregateOptions");
          spec.options = *so;
        }
        fields.push_back(arrow::field(agg.name, (spec.kind == kMean && spec.num_type == kNumDec128) ? in_schema.field(spec.col)->type()
                                                : spec.kind == kMean  ? arrow::float64()
                                                : spec.kind == kSum ? SumOutType(spec.num_type, &vtype)
                                                                    : in_schema.field(spec.col)->type()));
        if (spec.pair == 1) {
          const auto vt = in_schema.field(spec.col)->type();
          spec.out_type = vt;
          if (spec.out_type == nullptr) spec.out_type = fields.back()->type();
      aggs.push_back(spec);              // the hash_min half
          spec.kind = kMax;
          spec.pair = 2;                     // (the hash_max half is pushed below like every other aggregate)
          fields.back() = arrow::field(agg.name, arrow::struct_({arrow::field("min", vt), arrow::field("max", vt)}));
        }
      } else if (fn == "hash_first_last" || fn == "hash_list" || fn == "hash_distinct") {
        // hash_first_last: struct<first, last> of the two edge values (GroupedFirstLastImpl :738-925); hash_list: every value of
        // the group in row order, nulls included (GroupedListImpl :1858-1990); hash_distinct: the group's distinct values in
        // order of first appearance, CountOptions say whether a null is one of them (GroupedDistinctImpl :1480-1539)
        spec.kind = fn == "hash_first_last" ? kFirstLast : fn == "hash_list" ? kList : kDistinct;
        const int w = FixedByteWidth(vtype);
        const bool ok_width = spec.kind == kDistinct ? (w >= 1 && w <= 8) : (w == 1 || w == 2 || w == 4 || w == 8 || w == 16);
        if (!ok_width) {
          return Status::NotImplemented("aggregate_rocm: ", fn, " of ", vtype.ToString(), " columns (fixed-width values)");
        }
        if (agg.options != nullptr && spec.kind == kFirstLast) {
          const auto* so = dynamic_cast<const cp::ScalarAggregateOptions*>(agg.options.get());
          if (so == nullptr) return Status::TypeError("aggregate_rocm: hash_first_last takes ScalarAggregateOptions");
          spec.options = *so;
        }
        if (agg.options != nullptr && spec.kind == kDistinct) {
          const auto* co = dynamic_cast<const cp::CountOptions*>(agg.options.get());
          if (co == nullptr) return Status::TypeError("aggregate_rocm: hash_distinct takes CountOptions");
          spec.count_mode = co->mode == cp::CountOptions::ONLY_VALID ? ARX_COUNT_ONLY_VALID
                            : co->mode == cp::CountOptions::ONLY_NULL ? ARX_COUNT_ONLY_NULL : ARX_COUNT_ALL;
        }
        const auto& vt = in_schema.field(spec.col)->type();
        fields.push_back(arrow::field(agg.name, spec.kind == kFirstLast ? arrow::struct_({arrow::field("first", vt), arrow::field("last", vt)})
                                                                        : arrow::list(vt)));
      } else if (fn == "hash_variance" || fn == "hash_stddev" || fn == "hash_skew" || fn == "hash_kurtosis") {
        // GroupedStatisticImpl (kernels/hash_aggregate_numeric.cc:457-843): the moments of a group's valid values — two passes
        // over all rows of the node (mean, then the sums of (x - mean)^k in row order), arx_group_central_power +
        // arx_hash_moments_finalize.  The reference does the same per batch and merges the batches' moments: equal up to
        // floating-point rounding (its own tests compare approximately)
        spec.kind = fn == "hash_variance" ? kVariance : fn == "hash_stddev" ? kStddev : fn == "hash_skew" ? kSkew : kKurtosis;
        spec.num_type = SumNumType(vtype.id());
        if (spec.num_type < 0 || spec.num_type == kNumDec128) {
          return Status::NotImplemented("aggregate_rocm: ", fn, " of ", vtype.ToString(), " columns (integer or floating-point values)");
        }
        spec.options = cp::ScalarAggregateOptions(/*skip_nulls=*/true, /*min_count=*/0);   // (the defaults of VarianceOptions / SkewOptions)
        if (agg.options != nullptr) {
          if (spec.kind == kVariance || spec.kind == kStddev) {
            const auto* vo = dynamic_cast<const cp::VarianceOptions*>(agg.options.get());
            if (vo == nullptr) return Status::TypeError("aggregate_rocm: ", fn, " takes VarianceOptions");
            if (vo->ddof < 0) return Status::Invalid("aggregate_rocm: ", fn, " with a negative ddof");
            spec.ddof = vo->ddof;
            spec.options = cp::ScalarAggregateOptions(vo->skip_nulls, vo->min_count);
          } else {
            const auto* so = dynamic_cast<const cp::SkewOptions*>(agg.options.get());
            if (so == nullptr) return Status::TypeError("aggregate_rocm: ", fn, " takes SkewOptions");
            spec.biased = so->biased;
            spec.options = cp::ScalarAggregateOptions(so->skip_nulls, so->min_count);
          }
        }
        fields.push_back(arrow::field(agg.name, arrow::float64()));
      } else if (fn == "hash_product") {
        // GroupedProductImpl (kernels/hash_aggregate_numeric.cc:311-347): the product of a group's valid values in row order, in
        // the sum's accumulator type — arx_hash_product_consume
        spec.kind = kProduct;
        spec.num_type = SumNumType(vtype.id());
        if (spec.num_type < 0 || spec.num_type == kNumDec128) {
          return Status::NotImplemented("aggregate_rocm: hash_product of ", vtype.ToString(), " columns (integer or floating-point values)");
        }
        if (agg.options != nullptr) {
          const auto* so = dynamic_cast<const cp::ScalarAggregateOptions*>(agg.options.get());
          if (so == nullptr) return Status::TypeError("aggregate_rocm: hash_product takes ScalarAggregateOptions");
          spec.options = *so;
        }
        fields.push_back(arrow::field(agg.name, SumOutType(spec.num_type, &vtype)));
      } else if (fn == "hash_first" || fn == "hash_last" || fn == "hash_one") {
        // GroupedFirstLastImpl (kernels/hash_aggregate.cc:738-925) / GroupedOneImpl (:1556-1625): the first / last NON-NULL value
        // of the group in row order; hash_one's "any value" is, single-threaded, the first.  The rows are the batches in
        // batch.index order (Finish sorts them), so the answer is the reference's serial one whatever the thread count.
        spec.kind = fn == "hash_first" ? kFirst : fn == "hash_last" ? kLast : kOne;
        const int w = FixedByteWidth(vtype);
        if (w != 1 && w != 2 && w != 4 && w != 8 && w != 16) {
          return Status::NotImplemented("aggregate_rocm: ", fn, " of ", vtype.ToString(), " columns (fixed-width values of 1, 2, 4, 8 or 16 bytes)");
        }
        if (agg.options != nullptr && spec.kind != kOne) {
          const auto* so = dynamic_cast<const cp::ScalarAggregateOptions*>(agg.options.get());
          if (so == nullptr) return Status::TypeError("aggregate_rocm: ", fn, " takes ScalarAggregateOptions");
          spec.options = *so;
        }
        fields.push_back(arrow::field(agg.name, in_schema.field(spec.col)->type()));
      } else if (fn == "hash_any" || fn == "hash_all") {
        spec.kind = fn == "hash_any" ? kAny : kAll;
        if (vtype.id() != Type::BOOL) return Status::NotImplemented("aggregate_rocm: ", fn, " of ", vtype.ToString(), " columns (boolean values)");
        if (agg.options != nullptr) {
          const auto* so = dynamic_cast<const cp::ScalarAggregateOptions*>(agg.options.get());
          if (so == nullptr) return Status::TypeError("aggregate_rocm: ", fn, " takes ScalarAggregateOptions");
          spec.options = *so;
        }
        fields.push_back(arrow::field(agg.name, arrow::boolean()));
      } else {
        return Status::NotImplemented("aggregate_rocm: hash_sum / hash_mean / hash_min / hash_max / hash_min_max / hash_count / hash_count_all / "
                                      "hash_count_distinct / hash_distinct / hash_list / hash_any / hash_all / hash_first / hash_last / hash_first_last / hash_one / "
                                      "hash_product / hash_variance / hash_stddev / hash_skew / hash_kurtosis, got ", fn);
      }
      if (spec.out_type == nullptr) spec.out_type = fields.back()->type();
      aggs.push_back(spec);
    }
    return plan->EmplaceNode<RocmGroupByGeneralNode>(plan, std::move(inputs), arrow::schema(std::move(fields)),
                                                     std::move(key_cols), std::move(key_widths), std::move(aggs));
  }

  const char* kind_name() const override { return "RocmGroupByGeneralNode"; }

 private:
  Status Accept(int, cp::ExecBatch batch) override {
    if (batch.length > 0) {
      rows_ += batch.length;
      batches_[0].push_back(std::move(batch));
    }
    return Status::OK();
  }

  struct Staged {
    std::shared_ptr<Buffer> data, valid;   // valid == nullptr: no nulls
    int width = 0;                         // 0: boolean (`data` = its value bits, staged only when an aggregate reads them)
    bool want_bool_values = false;
  };

  // column `col` of every batch, concatenated into device buffers
  Status StageColumn(int col, hipStream_t st, Staged* out) {
    const auto& type = *inputs_[0]->output_schema()->field(col)->type();
    out->width = FixedByteWidth(type);
    const int64_t n = rows_;
    bool any_device = false, any_host = false, any_nulls = false;
    for (const auto& b : batches_[0]) {
      if (!b[col].is_array()) return Status::NotImplemented("aggregate_rocm: scalar columns");
      const ArrayData& a = *b[col].array();
      const bool dev = DataOnRocm(a);
      any_device = any_device || dev;
      any_host = any_host || !dev;
      any_nulls = any_nulls || (a.buffers[0] != nullptr && (dev ? a.null_count.load() != 0 : a.GetNullCount() != 0));
    }
    if (any_device && any_host) return Status::Invalid("aggregate_rocm: host and device-resident batches in one column");
    if (out->width > 0) {
      ARROW_ASSIGN_OR_RAISE(out->data, AllocDevice(n * out->width + 64));
    }
    const bool stage_bool = out->width == 0 && out->want_bool_values;
    if (stage_bool) {   // value bits, concatenated like a validity bitmap
      if (type.id() != Type::BOOL) return Status::Invalid("aggregate_rocm: value bits of a non-boolean column");
      ARROW_ASSIGN_OR_RAISE(out->data, AllocDevice(BitmapBytes(n)));
      HIP_RETURN_NOT_OK(hipMemsetAsync(reinterpret_cast<void*>(out->data->mutable_address()), 0, static_cast<size_t>(BitmapBytes(n)), st));
    }
    if (any_nulls) {
      ARROW_ASSIGN_OR_RAISE(out->valid, AllocDevice(BitmapBytes(n)));
      HIP_RETURN_NOT_OK(hipMemsetAsync(reinterpret_cast<void*>(out->valid->mutable_address()), 0, static_cast<size_t>(BitmapBytes(n)), st));
    }
    if (any_host) {
      // host batches: the reference's Concatenate, then one upload per buffer
      arrow::ArrayVector chunks;
      for (const auto& b : batches_[0]) chunks.push_back(b[col].make_array());
      ARROW_ASSIGN_OR_RAISE(auto whole, arrow::Concatenate(chunks, plan_->query_context()->memory_pool()));
      const ArrayData& w = *whole->data();
      if (out->width > 0) {
        HIP_RETURN_NOT_OK(hipMemcpyAsync(reinterpret_cast<void*>(out->data->mutable_address()),
                                         w.buffers[1]->data() + w.offset * out->width, static_cast<size_t>(n) * out->width,
                                         hipMemcpyHostToDevice, st));
      }
      if (any_nulls) {
        ARROW_ASSIGN_OR_RAISE(auto bits, arrow::internal::CopyBitmap(plan_->query_context()->memory_pool(), w.buffers[0]->data(), w.offset, n));
        HIP_RETURN_NOT_OK(hipMemcpyAsync(reinterpret_cast<void*>(out->valid->mutable_address()), bits->data(),
                                         static_cast<size_t>(arrow::bit_util::BytesForBits(n)), hipMemcpyHostToDevice, st));
        HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (`bits` goes out of scope)
      }
      if (stage_bool) {
        ARROW_ASSIGN_OR_RAISE(auto bits, arrow::internal::CopyBitmap(plan_->query_context()->memory_pool(), w.buffers[1]->data(), w.offset, n));
        HIP_RETURN_NOT_OK(hipMemcpyAsync(reinterpret_cast<void*>(out->data->mutable_address()), bits->data(),
                                         static_cast<size_t>(arrow::bit_util::BytesForBits(n)), hipMemcpyHostToDevice, st));
        HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
      }
      HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (the concatenated host array goes out of scope)
      return Status::OK();
    }
    // device batches: one launch for the values, one for the validity
    std::vector<ArxCopySeg> segs;
    std::vector<ArxBitSeg> bit_segs, value_bit_segs;
    uint64_t longest = 0;
    int64_t longest_rows = 0, at = 0;
    for (const auto& b : batches_[0]) {
      const ArrayData& a = *b[col].array();
      if (out->width > 0) {
        const auto* src = reinterpret_cast<const uint8_t*>(a.buffers[1]->address()) + a.offset * out->width;
        segs.push_back(ArxCopySeg{src, reinterpret_cast<uint8_t*>(out->data->mutable_address()) + at * out->width,
                                  static_cast<uint64_t>(a.length) * out->width});
        longest = std::max<uint64_t>(longest, static_cast<uint64_t>(a.length) * out->width);
      }
      if (any_nulls) {
        const void* bits = a.buffers[0] != nullptr && a.null_count.load() != 0 ? reinterpret_cast<const void*>(a.buffers[0]->address()) : nullptr;
        bit_segs.push_back(ArxBitSeg{bits, a.offset, reinterpret_cast<void*>(out->valid->mutable_address()), at, a.length});
        longest_rows = std::max(longest_rows, a.length);
      }
      if (stage_bool) {
        value_bit_segs.push_back(ArxBitSeg{reinterpret_cast<const void*>(a.buffers[1]->address()), a.offset,
                                           reinterpret_cast<void*>(out->data->mutable_address()), at, a.length});
        longest_rows = std::max(longest_rows, a.length);
      }
      at += a.length;
    }
    const size_t seg_bytes = segs.size() * sizeof(ArxCopySeg), bit_bytes = bit_segs.size() * sizeof(ArxBitSeg);
    const size_t value_bit_bytes = value_bit_segs.size() * sizeof(ArxBitSeg);
    ARROW_ASSIGN_OR_RAISE(auto table, AllocDevice(static_cast<int64_t>(seg_bytes + bit_bytes + value_bit_bytes) + 64));
    auto* d_table = reinterpret_cast<uint8_t*>(table->mutable_address());
    if (!segs.empty()) {
      HIP_RETURN_NOT_OK(hipMemcpyAsync(d_table, segs.data(), seg_bytes, hipMemcpyHostToDevice, st));
      ARROW_RETURN_NOT_OK(FromArx(arx_copy_segments(reinterpret_cast<const ArxCopySeg*>(d_table), static_cast<int64_t>(segs.size()), longest, st)));
    }
    if (!bit_segs.empty()) {
      HIP_RETURN_NOT_OK(hipMemcpyAsync(d_table + seg_bytes, bit_segs.data(), bit_bytes, hipMemcpyHostToDevice, st));
      ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy_segments(reinterpret_cast<const ArxBitSeg*>(d_table + seg_bytes),
                                                           static_cast<int64_t>(bit_segs.size()), longest_rows, st)));
    }
    if (!value_bit_segs.empty()) {
      HIP_RETURN_NOT_OK(hipMemcpyAsync(d_table + seg_bytes + bit_bytes, value_bit_segs.data(), value_bit_bytes, hipMemcpyHostToDevice, st));
      ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy_segments(reinterpret_cast<const ArxBitSeg*>(d_table + seg_bytes + bit_bytes),
                                                           static_cast<int64_t>(value_bit_segs.size()), longest_rows, st)));
    }
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (the segment tables are locals)
    return Status::OK();
  }

  static ArxSpan SpanOf(const Staged& s, int64_t n) {
    ArxSpan sp{};
    sp.validity = s.valid != nullptr ? reinterpret_cast<const void*>(s.valid->address()) : nullptr;
    sp.data = s.data != nullptr ? reinterpret_cast<const void*>(s.data->address()) : nullptr;
    sp.offset = 0;
    sp.length = n;
    sp.null_count = s.valid != nullptr ? arrow::kUnknownNullCount : 0;
    return sp;
  }

  template <typename T>
  static arrow::Result<std::shared_ptr<Buffer>> ZeroedDevice(int64_t count, hipStream_t st) {
    ARROW_ASSIGN_OR_RAISE(auto buf, AllocDevice(std::max<int64_t>(count, 1) * static_cast<int64_t>(sizeof(T))));
    HIP_RETURN_NOT_OK(hipMemsetAsync(reinterpret_cast<void*>(buf->mutable_address()), 0, static_cast<size_t>(std::max<int64_t>(count, 1)) * sizeof(T), st));
    return buf;
  }
  template <typename T>
  static T* Ptr(const std::shared_ptr<Buffer>& b) { return reinterpret_cast<T*>(b->mutable_address()); }

  // list<T> column from the groups' element counts (device) and the elements in group order (host): int32 offsets by a host
  // prefix sum.  keep = ARX_COUNT_ALL: every element; ONLY_VALID: the group's null element (one at most) is dropped;
  // ONLY_NULL: only that one is kept (GroupedDistinctImpl::Finalize's three modes)
  arrow::Result<arrow::Datum> ListsFromCounts(std::shared_ptr<arrow::DataType> list_type, const int64_t* d_counts, int64_t g,
                                              std::shared_ptr<ArrayData> values, hipStream_t st, int keep = ARX_COUNT_ALL) {
    arrow::MemoryPool* pool = plan_->query_context()->memory_pool();
    std::vector<int64_t> counts(static_cast<size_t>(std::max<int64_t>(g, 1)), 0);
    if (g > 0) HIP_RETURN_NOT_OK(hipMemcpyAsync(counts.data(), d_counts, static_cast<size_t>(g) * 8, hipMemcpyDeviceToHost, st));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    const uint8_t* vbits = values->buffers[0] != nullptr ? values->buffers[0]->data() : nullptr;
    if (keep != ARX_COUNT_ALL && !(keep == ARX_COUNT_ONLY_VALID && vbits == nullptr)) {
      // which elements stay (as a boolean mask for Arrow's own filter over the group-sized host array), and the new counts
      ARROW_ASSIGN_OR_RAISE(auto mask, arrow::AllocateBitmap(values->length, pool));
      int64_t pos = 0;
      for (int64_t i = 0; i < g; ++i) {
        int64_t kept = 0;
        for (int64_t j = 0; j < counts[static_cast<size_t>(i)]; ++j, ++pos) {
          const bool valid = vbits == nullptr || arrow::bit_util::GetBit(vbits, pos);
          const bool stay = keep == ARX_COUNT_ONLY_VALID ? valid : !valid;
          arrow::bit_util::SetBitTo(mask->mutable_data(), pos, stay);
          kept += stay ? 1 : 0;
        }
        counts[static_cast<size_t>(i)] = kept;
      }
      auto mask_arr = std::make_shared<arrow::BooleanArray>(values->length, std::move(mask));
      ARROW_ASSIGN_OR_RAISE(arrow::Datum filtered, cp::Filter(arrow::Datum(values), arrow::Datum(mask_arr), cp::FilterOptions(cp::FilterOptions::DROP)));
      values = filtered.array();
    }
    ARROW_ASSIGN_OR_RAISE(auto offsets, arrow::AllocateBuffer((g + 1) * 4, pool));
    auto* off = offsets->mutable_data_as<int32_t>();
    int64_t total = 0;
    off[0] = 0;
    for (int64_t i = 0; i < g; ++i) {
      total += counts[static_cast<size_t>(i)];
      if (total > std::numeric_limits<int32_t>::max()) return Status::CapacityError("aggregate_rocm: a list column of more than 2^31 - 1 elements");
      off[i + 1] = static_cast<int32_t>(total);
    }
    if (total != values->length) return Status::Invalid("aggregate_rocm: internal error (list offsets end at ", total, ", ", values->length, " elements)");
    return arrow::Datum(ArrayData::Make(std::move(list_type), g, {nullptr, std::move(offsets)}, {std::move(values)}, 0));
  }

  // validity bitmap (device words) + 8 bytes per group (device) -> one host array
  arrow::Result<arrow::Datum> ToHostColumn(std::shared_ptr<arrow::DataType> type, const void* d_values, int width,
                                           const void* d_bits, int64_t g, hipStream_t st) {
    arrow::MemoryPool* pool = plan_->query_context()->memory_pool();
    ARROW_ASSIGN_OR_RAISE(std::shared_ptr<Buffer> values, ColumnToHost(d_values, g * width, pool, st));
    std::shared_ptr<Buffer> bitmap;
    if (d_bits != nullptr && g > 0) {
      ARROW_ASSIGN_OR_RAISE(bitmap, arrow::AllocateBitmap(g, pool));
      HIP_RETURN_NOT_OK(hipMemcpyAsync(bitmap->mutable_data(), d_bits, static_cast<size_t>(arrow::bit_util::BytesForBits(g)),
                                       hipMemcpyDeviceToHost, st));
    }
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    int64_t null_count = 0;
    if (bitmap != nullptr) {
      null_count = g - arrow::internal::CountSetBits(bitmap->data(), 0, g);
      if (null_count == 0) bitmap = nullptr;
    }
    return arrow::Datum(ArrayData::Make(std::move(type), g, {std::move(bitmap), std::move(values)}, null_count));
  }

  // value bits + validity bits (device words) -> one host boolean array
  arrow::Result<arrow::Datum> ToHostBooleanColumn(const void* d_values, const void* d_bits, int64_t g, hipStream_t st) {
    arrow::MemoryPool* pool = plan_->query_context()->memory_pool();
    const size_t nbytes = static_cast<size_t>(arrow::bit_util::BytesForBits(g));
    ARROW_ASSIGN_OR_RAISE(std::shared_ptr<Buffer> values, arrow::AllocateBitmap(g, pool));
    ARROW_ASSIGN_OR_RAISE(std::shared_ptr<Buffer> bitmap, arrow::AllocateBitmap(g, pool));
    HIP_RETURN_NOT_OK(hipMemcpyAsync(values->mutable_data(), d_values, nbytes, hipMemcpyDeviceToHost, st));
    HIP_RETURN_NOT_OK(hipMemcpyAsync(bitmap->mutable_data(), d_bits, nbytes, hipMemcpyDeviceToHost, st));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    const int64_t null_count = g - arrow::internal::CountSetBits(bitmap->data(), 0, g);
    if (null_count == 0) bitmap = nullptr;
    return arrow::Datum(ArrayData::Make(arrow::boolean(), g, {std::move(bitmap), std::move(values)}, null_count));
  }

  Status Finish() override {
    std::vector<cp::ExecBatch>& batches = batches_[0];
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    const int64_t n = rows_;
    const int nk = static_cast<int>(key_cols_.size());
    std::vector<arrow::Datum> columns(nk + aggs_.size());
    int64_t g = 0;
    if (n >= (int64_t(1) << 31) - 64) return Status::NotImplemented("aggregate_rocm: more than 2^31 rows in one group-by");
    {
      // row order = batch.index order (the order of the source, whichever thread delivered a batch first): the ordered
      // aggregates (hash_first / hash_last / hash_one) and the row-order float sums mean THAT order; group ids then also
      // come out in order of first appearance in the table, as the reference's single-threaded Grouper numbers them
      if (!OrderBatchesByIndex(&batches)) {
        for (const Agg& a : aggs_) {
          if (a.kind == kFirst || a.kind == kLast || a.kind == kFirstLast || a.kind == kList) {
            return Status::NotImplemented("aggregate_rocm: hash_first / hash_last / hash_list over batches without an order (ExecBatch::index unset)");
          }
        }
      }
    }
    if (n > 0) {
      // ---- the columns the plan reads, once each
      std::map<int, Staged> staged;
      for (int j = 0; j < nk; ++j) {
        if (key_widths_[j] != 0) staged.emplace(key_cols_[j], Staged{});
      }
      // utf8 / binary key columns: Concatenate on the device (offsets rebased, host chunks uploaded), as order_by_rocm does
      std::map<int, std::shared_ptr<ArrayData>> var_keys;
      for (int j = 0; j < nk; ++j) {
        if (key_widths_[j] != 0 || var_keys.count(j) != 0) continue;
        std::vector<std::shared_ptr<ArrayData>> chunks;
        for (const auto& b : batches) {
          if (!b[key_cols_[j]].is_array()) return Status::NotImplemented("aggregate_rocm: scalar key columns");
          chunks.push_back(b[key_cols_[j]].array());
        }
        ARROW_ASSIGN_OR_RAISE(var_keys[j], ConcatOnDevice(inputs_[0]->output_schema()->field(key_cols_[j])->type(), chunks, st));
      }
      for (const Agg& a : aggs_) {
        if (a.col >= 0) staged.emplace(a.col, Staged{});
        if (a.kind == kAny || a.kind == kAll) staged[a.col].want_bool_values = true;
      }
      for (auto& kv : staged) ARROW_RETURN_NOT_OK(StageColumn(kv.first, st, &kv.second));
      std::vector<cp::ExecBatch>().swap(batches);   // the input may go
      // ---- Grouper: key rows -> dense ids in order of first appearance, through the chain of tables that
      // PlanGrouperLevels lays out (plugin/grouper_chain.inc); ONE table, initialised again for every level, since the
      // uniques of a level are read before the next level runs.
      const int64_t max_groups = n + 16;
      ARROW_ASSIGN_OR_RAISE(auto table_mem, AllocAligned(static_cast<int64_t>(arx_grouper_state_bytes(max_groups))));
      void* const table = table_mem.ptr;
      const size_t ws_bytes = arx_grouper_consume_workspace_bytes(n);
      ARROW_ASSIGN_OR_RAISE(auto ws_mem, AllocAligned(static_cast<int64_t>(ws_bytes)));
      void* const ws = ws_mem.ptr;
      // The Grouper's columns: a fixed-width key is one; a utf8 / binary key is its length and, first attempt, a 64-bit hash of
      // its bytes (arx_binary_key_hash) — ONE pass whatever the lengths; the groups are verified against their first rows'
      // bytes (arx_binary_key_verify), and only a batch in which different strings of one length share a hash takes the exact
      // chunk columns (BinaryKeyColumns; second attempt).
      std::vector<KeyColumn> cols;
      std::vector<int> key_of;   // per Grouper column: the key it is, -1 for a string's stand-ins
      std::map<int, ArxBinarySpan> var_spans;
      std::map<int, KeyColumn> var_lengths;
      std::map<int, int64_t> var_max_len;
      for (int j = 0; j < nk; ++j) {
        if (key_widths_[j] != 0) continue;
        const ArrayData& a = *var_keys[j];
        ArxBinarySpan bs{};
        bs.validity = a.buffers[0] != nullptr && a.null_count.load() != 0 ? reinterpret_cast<const void*>(a.buffers[0]->address()) : nullptr;
        bs.offsets = reinterpret_cast<const int32_t*>(a.buffers[1]->address());
        bs.data = a.buffers[2] != nullptr ? reinterpret_cast<const void*>(a.buffers[2]->address()) : nullptr;
        bs.offset = a.offset;
        bs.length = n;
        bs.null_count = bs.validity != nullptr ? arrow::kUnknownNullCount : 0;
        var_spans[j] = bs;
        ARROW_ASSIGN_OR_RAISE(var_lengths[j], BinaryKeyLengths(bs, n, st, &var_max_len[j]));
      }
      std::vector<std::vector<int>> levels;
      struct LevelUniques {
        std::vector<std::shared_ptr<Buffer>> vals, bits;   // one per Grouper column of the level (nullptr: not a key column itself)
        std::vector<int64_t> nulls;
        std::shared_ptr<Buffer> prev_ids;                  // [groups of this level] id at the level before (levels >= 1)
        int64_t groups = 0;
      };
      std::vector<LevelUniques> uniq;
      std::shared_ptr<Buffer> ids_buf;
      const int hash_bits = static_cast<int>(g_string_key_hash_bits.load());
      for (int attempt = (var_keys.empty() || hash_bits <= 0) ? 1 : 0; attempt < 2; ++attempt) {
      const bool hashed = attempt == 0;
      cols.clear();
      key_of.clear();
      for (int j = 0; j < nk; ++j) {
        if (key_widths_[j] != 0) {
          cols.push_back(KeyColumn{SpanOf(staged[key_cols_[j]], n), key_widths_[j], false, {}});
        } else if (hashed) {
          cols.push_back(var_lengths[j]);
          ARROW_ASSIGN_OR_RAISE(auto hash, AllocDevice(n * 8 + 64));
          ARROW_RETURN_NOT_OK(FromArx(arx_binary_key_hash(&var_spans[j], hash_bits, Ptr<uint64_t>(hash), st)));
          cols.push_back(KeyColumn{ArxSpan{nullptr, Ptr<void>(hash), 0, n, 0}, 8, false, {hash}});
        } else {
          ARROW_RETURN_NOT_OK(BinaryKeyColumns(var_spans[j], n, var_lengths[j], var_max_len[j], st, &cols));
        }
        key_of.resize(cols.size(), key_widths_[j] != 0 ? j : -1);
      }
      levels = PlanGrouperLevels(cols);
      uniq.assign(levels.size(), LevelUniques{});
      ids_buf = nullptr;
      for (size_t s = 0; s < levels.size(); ++s) {
        ARROW_RETURN_NOT_OK(FromArx(arx_grouper_init(table, max_groups, st)));
        std::vector<ArxSpan> key_spans;
        std::vector<int> widths;
        if (s > 0) {
          ArxSpan prev{};
          prev.data = Ptr<void>(ids_buf);
          prev.length = n;
          key_spans.push_back(prev);
          widths.push_back(4);
        }
        for (int v : levels[s]) {
          key_spans.push_back(cols[v].span);
          widths.push_back(cols[v].width);
        }
        const int lk = static_cast<int>(widths.size());
        ARROW_ASSIGN_OR_RAISE(auto next_ids, AllocDevice(n * 4 + 64));
        ARROW_RETURN_NOT_OK(FromArx(arx_grouper_consume(table, max_groups, key_spans.data(), widths.data(), lk, ws, ws_bytes,
                                                        Ptr<uint32_t>(next_ids), st)));
        ids_buf = std::move(next_ids);   // (the previous level's ids were this consume's first key column: in-order stream)
        LevelUniques& u = uniq[s];
        ARROW_RETURN_NOT_OK(FromArx(arx_grouper_num_groups(table, &u.groups, st)));
        for (int c = 0; c < lk; ++c) {
          const bool prev_col = s > 0 && c == 0;
          const int v = prev_col ? -1 : levels[s][c - (s > 0 ? 1 : 0)];
          if (!prev_col && key_of[v] < 0) {   // a string's stand-in: its uniques come from the first rows below
            u.vals.push_back(nullptr);
            u.bits.push_back(nullptr);
            u.nulls.push_back(0);
            continue;
          }
          ARROW_ASSIGN_OR_RAISE(auto vals, AllocDevice(std::max<int64_t>(u.groups, 1) * widths[c] + 64));
          ARROW_ASSIGN_OR_RAISE(auto bits, AllocDevice(BitmapBytes(u.groups)));
          int64_t nulls = 0;
          ARROW_RETURN_NOT_OK(FromArx(arx_grouper_get_uniques(table, max_groups, widths.data(), lk, c, Ptr<void>(vals),
                                                              Ptr<uint8_t>(bits), &nulls, st)));
          if (prev_col) {
            u.prev_ids = std::move(vals);
          } else {
            u.vals.push_back(std::move(vals));
            u.bits.push_back(std::move(bits));
            u.nulls.push_back(nulls);
          }
        }
        HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
      }
      if (!hashed) break;
      // the hashed groups are the exact groups unless some row's bytes differ from its group's first row's
      {
        const int64_t hg = uniq.back().groups;
        ARROW_ASSIGN_OR_RAISE(auto first_rows, AllocDevice(std::max<int64_t>(hg, 1) * 4 + 64));
        ARROW_RETURN_NOT_OK(FromArx(arx_group_first_rows(Ptr<uint32_t>(ids_buf), n, hg, Ptr<uint32_t>(first_rows), st)));
        int64_t mismatches = 0;
        for (auto& kv : var_spans) {
          int64_t bad = 0;
          ARROW_RETURN_NOT_OK(FromArx(arx_binary_key_verify(&kv.second, Ptr<uint32_t>(ids_buf), Ptr<uint32_t>(first_rows), &bad, ws, st)));
          mismatches += bad;
        }
        if (mismatches == 0) break;
        g_string_key_hash_collisions.fetch_add(1, std::memory_order_relaxed);
      }
      }   // attempts
      cols.clear();   // (the strings' stand-ins go back to the pool)
      g = uniq.back().groups;
      const uint32_t* ids = Ptr<uint32_t>(ids_buf);
      CountGpu(kFnHashSum);
      // ---- key columns: GetUniques.  The last level's are in final id order; an earlier level's are gathered through
      // the composed maps final id -> level id (each level kept its groups' ids at the level before)
      const auto& in_schema = *inputs_[0]->output_schema();
      std::shared_ptr<Buffer> to_level;   // nullptr: the identity
      for (size_t s = levels.size(); s-- > 0;) {
        const LevelUniques& u = uniq[s];
        ArxSpan map{};
        map.data = to_level != nullptr ? Ptr<void>(to_level) : nullptr;
        map.length = g;
        for (size_t c = 0; c < levels[s].size(); ++c) {
          if (u.vals[c] == nullptr) continue;
          const int j = key_of[levels[s][c]];
          const int w = key_widths_[j];
          const auto& type = in_schema.field(key_cols_[j])->type();
          if (to_level == nullptr) {
            ARROW_ASSIGN_OR_RAISE(columns[j], ToHostColumn(type, Ptr<void>(u.vals[c]), w,
                                                           u.nulls[c] != 0 ? Ptr<void>(u.bits[c]) : nullptr, g, st));
            continue;
          }
          ArxSpan src{};
          src.data = Ptr<void>(u.vals[c]);
          src.validity = u.nulls[c] != 0 ? Ptr<void>(u.bits[c]) : nullptr;
          src.length = u.groups;
          src.null_count = u.nulls[c] != 0 ? arrow::kUnknownNullCount : 0;
          ARROW_ASSIGN_OR_RAISE(auto vals, AllocDevice(std::max<int64_t>(g, 1) * w + 64));
          std::shared_ptr<Buffer> bits;
          if (u.nulls[c] != 0) {
            ARROW_ASSIGN_OR_RAISE(bits, AllocDevice(BitmapBytes(g)));
            HIP_RETURN_NOT_OK(hipMemsetAsync(Ptr<void>(bits), 0, static_cast<size_t>(BitmapBytes(g)), st));
          }
          ARROW_RETURN_NOT_OK(FromArx(arx_take(&src, w, &map, ARX_UINT32, Ptr<void>(vals), bits != nullptr ? Ptr<void>(bits) : nullptr,
                                               nullptr, st)));
          ARROW_ASSIGN_OR_RAISE(columns[j], ToHostColumn(type, Ptr<void>(vals), w, bits != nullptr ? Ptr<void>(bits) : nullptr, g, st));
        }
        if (s > 0) {
          if (to_level == nullptr) {
            to_level = u.prev_ids;
          } else {
            ArxSpan src{};
            src.data = Ptr<void>(u.prev_ids);
            src.length = u.groups;
            ARROW_ASSIGN_OR_RAISE(auto composed, AllocDevice(std::max<int64_t>(g, 1) * 4 + 64));
            ARROW_RETURN_NOT_OK(FromArx(arx_take(&src, 4, &map, ARX_UINT32, Ptr<void>(composed), nullptr, nullptr, st)));
            to_level = std::move(composed);
          }
        }
      }
      // utf8 / binary key columns: the unique strings are the strings of every group's FIRST row (array_take's binary
      // gather by uint32 row numbers), copied back buffer by buffer
      if (!var_keys.empty()) {
        ARROW_ASSIGN_OR_RAISE(auto first_rows, AllocDevice(std::max<int64_t>(g, 1) * 4 + 64));
        ARROW_RETURN_NOT_OK(FromArx(arx_group_first_rows(ids, n, g, Ptr<uint32_t>(first_rows), st)));
        ArxSpan di{};
        di.data = Ptr<void>(first_rows);
        di.length = g;
        for (auto& kv : var_keys) {
          const int j = kv.first;
          ArrayData taken;
          ARROW_RETURN_NOT_OK(BinaryTakeOnDevice(var_spans[j], di, ARX_UINT32, st, &taken));
          taken.type = in_schema.field(key_cols_[j])->type();
          auto* pool = plan_->query_context()->memory_pool();
          for (auto& buf : taken.buffers) {
            if (buf == nullptr) continue;
            ARROW_ASSIGN_OR_RAISE(std::shared_ptr<Buffer> host, ColumnToHost(Ptr<void>(buf), buf->size(), pool, st));
            buf = std::move(host);
          }
          HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
          if (taken.null_count.load() == 0) taken.buffers[0] = nullptr;
          columns[j] = arrow::Datum(std::make_shared<ArrayData>(std::move(taken)));
        }
      }
      // ---- the aggregates: dense per-group state, one consume over all rows each
      ARROW_ASSIGN_OR_RAISE(auto bits_buf, AllocDevice(BitmapBytes(g)));
      ARROW_ASSIGN_OR_RAISE(auto flag_buf, ZeroedDevice<int64_t>(4, st));
      for (size_t ai = 0; ai < aggs_.size(); ++ai) {
        const Agg& a = aggs_[ai];
        arrow::Datum& out = columns[nk + ai];
        if (a.kind == kCount || a.kind == kCountAll) {
          ARROW_ASSIGN_OR_RAISE(auto counts, ZeroedDevice<int64_t>(g, st));
          const Staged* col = a.kind == kCount ? &staged[a.col] : nullptr;
          const void* bits = col != nullptr && col->valid != nullptr ? reinterpret_cast<const void*>(col->valid->address()) : nullptr;
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_count_consume(bits, 0, bits != nullptr ? arrow::kUnknownNullCount : 0,
                                                             a.kind == kCountAll ? ARX_COUNT_ALL : a.count_mode, ids, n,
                                                             Ptr<int64_t>(counts), st)));
          ARROW_ASSIGN_OR_RAISE(out, ToHostColumn(arrow::int64(), Ptr<void>(counts), 8, nullptr, g, st));
          continue;
        }
        if (a.kind == kCountDistinct || a.kind == kDistinct) {
          // a second device Grouper over (value, group id): its groups are the distinct pairs, its uniques say which group a
          // pair belongs to and whether its value is null (GroupedCountDistinctImpl::Finalize :1441-1468)
          const Staged& col = staged[a.col];
          const int64_t max_pairs = n + 16;
          ARROW_ASSIGN_OR_RAISE(auto pair_table_buf, AllocAligned(static_cast<int64_t>(arx_grouper_state_bytes(max_pairs))));
          void* pair_table = pair_table_buf.ptr;
          ARROW_RETURN_NOT_OK(FromArx(arx_grouper_init(pair_table, max_pairs, st)));
          const size_t pws_bytes = arx_grouper_consume_workspace_bytes(n);
          ARROW_ASSIGN_OR_RAISE(auto pws_buf, AllocAligned(static_cast<int64_t>(pws_bytes)));
          void* pws = pws_buf.ptr;
          ArxSpan pair_cols[2] = {SpanOf(col, n), ArxSpan{nullptr, ids, 0, n, 0}};
          const int32_t pair_widths[2] = {col.width, 4};
          ARROW_ASSIGN_OR_RAISE(auto pair_ids, AllocDevice(n * 4 + 64));
          ARROW_RETURN_NOT_OK(FromArx(arx_grouper_consume(pair_table, max_pairs, pair_cols, pair_widths, 2, pws, pws_bytes,
                                                          Ptr<uint32_t>(pair_ids), st)));
          int64_t pairs = 0;
          ARROW_RETURN_NOT_OK(FromArx(arx_grouper_num_groups(pair_table, &pairs, st)));
          ARROW_ASSIGN_OR_RAISE(auto pair_vals, AllocDevice(std::max<int64_t>(pairs, 1) * col.width + 64));
          ARROW_ASSIGN_OR_RAISE(auto pair_bits, AllocDevice(BitmapBytes(pairs)));
          ARROW_ASSIGN_OR_RAISE(auto pair_groups, AllocDevice(std::max<int64_t>(pairs, 1) * 4 + 64));
          ARROW_ASSIGN_OR_RAISE(auto unused_bits, AllocDevice(BitmapBytes(pairs)));
          int64_t null_pairs = 0, unused = 0;
          ARROW_RETURN_NOT_OK(FromArx(arx_grouper_get_uniques(pair_table, max_pairs, pair_widths, 2, 0, Ptr<void>(pair_vals),
                                                              Ptr<uint8_t>(pair_bits), &null_pairs, st)));
          ARROW_RETURN_NOT_OK(FromArx(arx_grouper_get_uniques(pair_table, max_pairs, pair_widths, 2, 1, Ptr<void>(pair_groups),
                                                              Ptr<uint8_t>(unused_bits), &unused, st)));
          ARROW_ASSIGN_OR_RAISE(auto counts, ZeroedDevice<int64_t>(g, st));
          const void* bits = null_pairs != 0 ? Ptr<void>(pair_bits) : nullptr;
          if (a.kind == kDistinct) {
            // GroupedDistinctImpl::Finalize (:1480-1539): the distinct pairs grouped by their group id in order of first
            // appearance (MakeGroupings / ApplyGroupings = a stable partition by group), then ONLY_VALID drops a group's null,
            // ONLY_NULL keeps nothing else.  Here: the pairs stably sorted by group id, one take, and the mode applied to the
            // (group-sized) host result
            std::shared_ptr<ArrayData> values_host = ArrayData::Make(inputs_[0]->output_schema()->field(a.col)->type(), 0, {nullptr, nullptr}, 0);
            if (pairs > 0) {
              ARROW_RETURN_NOT_OK(FromArx(arx_hash_count_consume(nullptr, 0, 0, ARX_COUNT_ALL, Ptr<uint32_t>(pair_groups), pairs, Ptr<int64_t>(counts), st)));
              const size_t sws_bytes = arx_sort_indices_workspace_bytes(pairs);
              ARROW_ASSIGN_OR_RAISE(auto sws, AllocAligned(static_cast<int64_t>(sws_bytes)));
              ARROW_ASSIGN_OR_RAISE(auto perm, AllocDevice(pairs * 8 + 64));
              const ArxSpan gkeys{nullptr, Ptr<void>(pair_groups), 0, pairs, 0};
              ARROW_RETURN_NOT_OK(FromArx(arx_sort_indices(&gkeys, ARX_KEY_UINT32, ARX_SORT_ASCENDING, ARX_NULLS_AT_END,
                                                           sws.ptr, sws_bytes,
                                                           Ptr<uint64_t>(perm), st)));
              ARROW_ASSIGN_OR_RAISE(auto dvals, AllocDevice(pairs * col.width + 64));
              std::shared_ptr<Buffer> dbits;
              if (bits != nullptr) {
                ARROW_ASSIGN_OR_RAISE(dbits, AllocDevice(BitmapBytes(pairs)));
                HIP_RETURN_NOT_OK(hipMemsetAsync(Ptr<void>(dbits), 0, static_cast<size_t>(BitmapBytes(pairs)), st));
              }
              ArxSpan src{bits, Ptr<void>(pair_vals), 0, pairs, bits != nullptr ? arrow::kUnknownNullCount : 0};
              ArxSpan idx{nullptr, Ptr<void>(perm), 0, pairs, 0};
              ARROW_RETURN_NOT_OK(FromArx(arx_take(&src, col.width, &idx, ARX_UINT64, Ptr<void>(dvals), dbits != nullptr ? Ptr<void>(dbits) : nullptr, nullptr, st)));
              ARROW_ASSIGN_OR_RAISE(arrow::Datum vh, ToHostColumn(inputs_[0]->output_schema()->field(a.col)->type(), Ptr<void>(dvals), col.width,
                                                                  dbits != nullptr ? Ptr<void>(dbits) : nullptr, pairs, st));
              values_host = vh.array();
            }
            ARROW_ASSIGN_OR_RAISE(out, ListsFromCounts(a.out_type, Ptr<int64_t>(counts), g, values_host, st,
                                                       a.count_mode));
            continue;
          }
          if (pairs > 0) {
            ARROW_RETURN_NOT_OK(FromArx(arx_hash_count_consume(bits, 0, bits != nullptr ? arrow::kUnknownNullCount : 0, a.count_mode,
                                                               Ptr<uint32_t>(pair_groups), pairs, Ptr<int64_t>(counts), st)));
          }
          ARROW_ASSIGN_OR_RAISE(out, ToHostColumn(arrow::int64(), Ptr<void>(counts), 8, nullptr, g, st));
          continue;
        }
        if (a.kind == kFirst || a.kind == kLast || a.kind == kOne || a.kind == kFirstLast) {
          // the row of every group's first / last non-null value (arx_group_edge_rows), then ONE take; the slot is valid where
          // the group has a non-null value and — skip_nulls = false — no null row comes before (after) it
          // (GroupedFirstLastImpl::Finalize :864-905)
          const Staged& col = staged[a.col];
          const void* vbits = col.valid != nullptr ? reinterpret_cast<const void*>(col.valid->address()) : nullptr;
          auto edge = [&](bool last) -> arrow::Result<arrow::Datum> {
          arrow::Datum out;
          ARROW_ASSIGN_OR_RAISE(auto rows, AllocDevice(std::max<int64_t>(g, 1) * 4 + 64));
          ARROW_ASSIGN_OR_RAISE(auto has, AllocDevice(BitmapBytes(g)));
          ARROW_RETURN_NOT_OK(FromArx(arx_group_edge_rows(ids, vbits, 0, n, g, last ? 1 : 0, Ptr<uint32_t>(rows), Ptr<void>(has), st)));
          if (a.kind != kOne && !a.options.skip_nulls && vbits != nullptr) {
            // the group's first (last) row of ANY validity: where it differs from the first (last) valid row, a null came first
            ARROW_ASSIGN_OR_RAISE(auto any_rows, AllocDevice(std::max<int64_t>(g, 1) * 4 + 64));
            ARROW_ASSIGN_OR_RAISE(auto any_has, AllocDevice(BitmapBytes(g)));
            ARROW_RETURN_NOT_OK(FromArx(arx_group_edge_rows(ids, nullptr, 0, n, g, last ? 1 : 0, Ptr<uint32_t>(any_rows), Ptr<void>(any_has), st)));
            ARROW_ASSIGN_OR_RAISE(auto same, AllocDevice(BitmapBytes(g)));
            ARROW_RETURN_NOT_OK(FromArx(arx_compare_numeric(ARX_CMP_EQUAL, ARX_NUM_UINT32, Ptr<void>(rows), nullptr, Ptr<void>(any_rows), nullptr,
                                                            g, Ptr<uint64_t>(same), st)));
            ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_and(Ptr<void>(has), 0, Ptr<void>(same), 0, g, Ptr<void>(has), st)));
          }
          const int w = col.width;
          ARROW_ASSIGN_OR_RAISE(auto vals_out, AllocDevice(std::max<int64_t>(g, 1) * w + 64));
          ARROW_ASSIGN_OR_RAISE(auto bits_out, AllocDevice(BitmapBytes(g)));
          HIP_RETURN_NOT_OK(hipMemsetAsync(Ptr<void>(bits_out), 0, static_cast<size_t>(BitmapBytes(g)), st));
          ArxSpan src = SpanOf(col, n);
          ArxSpan idx{Ptr<void>(has), Ptr<void>(rows), 0, g, arrow::kUnknownNullCount};
          ARROW_RETURN_NOT_OK(FromArx(arx_take(&src, w, &idx, ARX_UINT32, Ptr<void>(vals_out), Ptr<void>(bits_out), nullptr, st)));
          ARROW_ASSIGN_OR_RAISE(out, ToHostColumn(inputs_[0]->output_schema()->field(a.col)->type(), Ptr<void>(vals_out), w, Ptr<void>(bits_out), g, st));
          return out;
          };
          if (a.kind == kFirstLast) {
            ARROW_ASSIGN_OR_RAISE(arrow::Datum first, edge(false));
            ARROW_ASSIGN_OR_RAISE(arrow::Datum last, edge(true));
            out = arrow::Datum(ArrayData::Make(a.out_type, g, {nullptr}, {first.array(), last.array()}, 0));
          } else {
            ARROW_ASSIGN_OR_RAISE(out, edge(a.kind == kLast));
          }
          continue;
        }
        if (a.kind == kList) {
          // every value of a group in row order: the rows stably sorted by group id, one take, the offsets from the groups' row counts
          const Staged& col = staged[a.col];
          const int w = col.width;
          const size_t sws_bytes = arx_sort_indices_workspace_bytes(n);
          ARROW_ASSIGN_OR_RAISE(auto sws, AllocAligned(static_cast<int64_t>(sws_bytes)));
          ARROW_ASSIGN_OR_RAISE(auto perm, AllocDevice(n * 8 + 64));
          const ArxSpan gkeys{nullptr, ids, 0, n, 0};
          ARROW_RETURN_NOT_OK(FromArx(arx_sort_indices(&gkeys, ARX_KEY_UINT32, ARX_SORT_ASCENDING, ARX_NULLS_AT_END,
                                                       sws.ptr, sws_bytes,
                                                       Ptr<uint64_t>(perm), st)));
          ARROW_ASSIGN_OR_RAISE(auto lvals, AllocDevice(n * w + 64));
          std::shared_ptr<Buffer> lbits;
          if (col.valid != nullptr) {
            ARROW_ASSIGN_OR_RAISE(lbits, AllocDevice(BitmapBytes(n)));
            HIP_RETURN_NOT_OK(hipMemsetAsync(Ptr<void>(lbits), 0, static_cast<size_t>(BitmapBytes(n)), st));
          }
          ArxSpan src = SpanOf(col, n);
          ArxSpan idx{nullptr, Ptr<void>(perm), 0, n, 0};
          ARROW_RETURN_NOT_OK(FromArx(arx_take(&src, w, &idx, ARX_UINT64, Ptr<void>(lvals), lbits != nullptr ? Ptr<void>(lbits) : nullptr, nullptr, st)));
          ARROW_ASSIGN_OR_RAISE(auto counts, ZeroedDevice<int64_t>(g, st));
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_count_consume(nullptr, 0, 0, ARX_COUNT_ALL, ids, n, Ptr<int64_t>(counts), st)));
          ARROW_ASSIGN_OR_RAISE(arrow::Datum values_host, ToHostColumn(inputs_[0]->output_schema()->field(a.col)->type(), Ptr<void>(lvals), w,
                                                                       lbits != nullptr ? Ptr<void>(lbits) : nullptr, n, st));
          ARROW_ASSIGN_OR_RAISE(out, ListsFromCounts(a.out_type, Ptr<int64_t>(counts), g,
                                                     values_host.array(), st));
          continue;
        }
        if (a.kind == kAny || a.kind == kAll) {
          // GroupedBooleanAggregator (kernels/hash_aggregate.cc:1232-1398) from three dense counts per group: valid rows,
          // null rows, valid rows whose value is true — the same kernels as the hash_any / hash_all vtables
          const Staged& col = staged[a.col];
          const void* valid_bits = col.valid != nullptr ? reinterpret_cast<const void*>(col.valid->address()) : nullptr;
          const void* true_bits = reinterpret_cast<const void*>(col.data->address());
          ARROW_ASSIGN_OR_RAISE(auto n_valid, ZeroedDevice<int64_t>(g, st));
          ARROW_ASSIGN_OR_RAISE(auto n_null, ZeroedDevice<int64_t>(g, st));
          ARROW_ASSIGN_OR_RAISE(auto n_true, ZeroedDevice<int64_t>(g, st));
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_count_consume(valid_bits, 0, valid_bits != nullptr ? arrow::kUnknownNullCount : 0,
                                                             ARX_COUNT_ONLY_VALID, ids, n, Ptr<int64_t>(n_valid), st)));
          std::shared_ptr<Buffer> both;
          if (valid_bits != nullptr) {
            ARROW_RETURN_NOT_OK(FromArx(arx_hash_count_consume(valid_bits, 0, arrow::kUnknownNullCount, ARX_COUNT_ONLY_NULL, ids, n,
                                                               Ptr<int64_t>(n_null), st)));
            ARROW_ASSIGN_OR_RAISE(both, AllocDevice(BitmapBytes(n)));
            ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_and(valid_bits, 0, true_bits, 0, n, Ptr<void>(both), st)));
            true_bits = Ptr<void>(both);
          }
          // (null_count = -1: "has a bitmap, count the set bits" — the bitmap here is the predicate, not a validity)
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_count_consume(true_bits, 0, -1, ARX_COUNT_ONLY_VALID, ids, n, Ptr<int64_t>(n_true), st)));
          ARROW_ASSIGN_OR_RAISE(auto value_bits, AllocDevice(BitmapBytes(g)));
          HIP_RETURN_NOT_OK(hipMemsetAsync(Ptr<void>(flag_buf), 0, 32, st));
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_bool_finalize(Ptr<int64_t>(n_valid), Ptr<int64_t>(n_null), Ptr<int64_t>(n_true), g,
                                                             a.kind == kAll ? 1 : 0, a.options.skip_nulls ? 1 : 0, a.options.min_count,
                                                             Ptr<void>(value_bits), Ptr<void>(bits_buf), Ptr<int64_t>(flag_buf), st)));
          ARROW_ASSIGN_OR_RAISE(out, ToHostBooleanColumn(Ptr<void>(value_bits), Ptr<void>(bits_buf), g, st));
          continue;
        }
        ArxSpan vals = SpanOf(staged[a.col], n);
        std::shared_ptr<Buffer> wide_buf;
        if (a.num_type == kNumDec128 && (a.kind == kMin || a.kind == kMax)) {
          // decimal128 extrema: the rows sorted by group id, one owner per group (arx_hash_minmax_dec128_consume)
          ARROW_ASSIGN_OR_RAISE(auto dseen, ZeroedDevice<uint32_t>(g, st));
          ARROW_ASSIGN_OR_RAISE(auto dmins, AllocDevice(std::max<int64_t>(g, 1) * 16));
          ARROW_ASSIGN_OR_RAISE(auto dmaxs, AllocDevice(std::max<int64_t>(g, 1) * 16));
          HIP_RETURN_NOT_OK(hipMemsetAsync(Ptr<void>(dmins), 0, static_cast<size_t>(std::max<int64_t>(g, 1)) * 16, st));   // (a group without a value: a null slot, zero bytes under it)
          HIP_RETURN_NOT_OK(hipMemsetAsync(Ptr<void>(dmaxs), 0, static_cast<size_t>(std::max<int64_t>(g, 1)) * 16, st));
          const size_t dws_bytes = arx_hash_minmax_dec128_workspace_bytes(n);
          ARROW_ASSIGN_OR_RAISE(auto dws, AllocDevice(static_cast<int64_t>(dws_bytes) + 256));
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_minmax_dec128_consume(&vals, ids, n, Ptr<void>(dws), dws_bytes + 256, Ptr<void>(dmins),
                                                                     Ptr<void>(dmaxs), Ptr<uint32_t>(dseen), st)));
          HIP_RETURN_NOT_OK(hipMemsetAsync(Ptr<void>(flag_buf), 0, 32, st));
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_minmax_dec128_finalize(Ptr<uint32_t>(dseen), g, a.options.skip_nulls ? 1 : 0, Ptr<void>(bits_buf),
                                                                      Ptr<int64_t>(flag_buf), st)));
          ARROW_ASSIGN_OR_RAISE(out, ToHostColumn(a.out_type,
                                                  Ptr<void>(a.kind == kMin ? dmins : dmaxs), 16, Ptr<void>(bits_buf), g, st));
          continue;
        }
        if (a.num_type == kNumDec128) {
          // decimal128 sums: 128 bits per group modulo 2^128, two atomics a row (arx_hash_sum_dec128_consume)
          ARROW_ASSIGN_OR_RAISE(auto dseen, ZeroedDevice<uint32_t>(g, st));
          ARROW_ASSIGN_OR_RAISE(auto dlo, ZeroedDevice<int64_t>(g, st));
          ARROW_ASSIGN_OR_RAISE(auto dhi, ZeroedDevice<int64_t>(g, st));
          ARROW_ASSIGN_OR_RAISE(auto dcounts, ZeroedDevice<int64_t>(g, st));
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_sum_dec128_consume(&vals, 0, 0, 0, ids, n, Ptr<uint64_t>(dlo), Ptr<uint64_t>(dhi),
                                                                  Ptr<int64_t>(dcounts), Ptr<uint32_t>(dseen), st)));
          ARROW_ASSIGN_OR_RAISE(auto packed, AllocDevice(std::max<int64_t>(g, 1) * 16));
          ARROW_RETURN_NOT_OK(FromArx(arx_dec128_pack(Ptr<uint64_t>(dlo), Ptr<uint64_t>(dhi), g, Ptr<void>(packed), st)));
          HIP_RETURN_NOT_OK(hipMemsetAsync(Ptr<void>(flag_buf), 0, 32, st));
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_sum_i64_finalize(Ptr<int64_t>(dcounts), Ptr<uint32_t>(dseen), g, a.options.skip_nulls ? 1 : 0,
                                                                a.options.min_count, Ptr<void>(bits_buf), Ptr<int64_t>(flag_buf), st)));
          ARROW_ASSIGN_OR_RAISE(out, ToHostColumn(a.out_type, Ptr<void>(packed), 16,
                                                  Ptr<void>(bits_buf), g, st));
          if (a.kind == kMean && g > 0) {   // GroupedMeanImpl::DoMean for decimals: truncating division + rounding, on the host
            std::vector<int64_t> host_counts(static_cast<size_t>(g));
            HIP_RETURN_NOT_OK(hipMemcpyAsync(host_counts.data(), Ptr<void>(dcounts), static_cast<size_t>(g) * 8, hipMemcpyDeviceToHost, st));
            HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
            ARROW_RETURN_NOT_OK(DecimalMeansInPlace(out.array()->buffers[1]->mutable_data(), host_counts.data(), g, a.options.min_count));
          }
          continue;
        }
        if (a.kind == kProduct) {
          ARROW_ASSIGN_OR_RAISE(auto pseen, ZeroedDevice<uint32_t>(g, st));
          ARROW_ASSIGN_OR_RAISE(auto pcounts, ZeroedDevice<int64_t>(g, st));
          ARROW_ASSIGN_OR_RAISE(auto prods, AllocDevice(std::max<int64_t>(g, 1) * 8));
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_product_init(Ptr<void>(prods), a.num_type, g, st)));
          const size_t pws_bytes = arx_hash_sum_float_workspace_bytes(n);
          ARROW_ASSIGN_OR_RAISE(auto pws, AllocDevice(static_cast<int64_t>(pws_bytes) + 256));
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_product_consume(&vals, a.num_type, ids, n, Ptr<void>(pws), pws_bytes + 256, Ptr<void>(prods),
                                                               Ptr<int64_t>(pcounts), Ptr<uint32_t>(pseen), st)));
          HIP_RETURN_NOT_OK(hipMemsetAsync(Ptr<void>(flag_buf), 0, 32, st));
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_sum_i64_finalize(Ptr<int64_t>(pcounts), Ptr<uint32_t>(pseen), g, a.options.skip_nulls ? 1 : 0,
                                                                a.options.min_count, Ptr<void>(bits_buf), Ptr<int64_t>(flag_buf), st)));
          ARROW_ASSIGN_OR_RAISE(out, ToHostColumn(a.out_type, Ptr<void>(prods), 8,
                                                  Ptr<void>(bits_buf), g, st));
          continue;
        }
        if (a.kind == kVariance || a.kind == kStddev || a.kind == kSkew || a.kind == kKurtosis) {
          int ftype = a.num_type;
          if (!NumIsFloat(ftype)) {   // integers: ToDouble of every value (:537), once
            ARROW_ASSIGN_OR_RAISE(wide_buf, AllocDevice(std::max<int64_t>(n, 1) * 8));
            ARROW_RETURN_NOT_OK(FromArx(arx_cast_numeric(&vals, a.num_type, ARX_NUM_FLOAT64, /*allow_int_overflow=*/1, /*allow_float_truncate=*/1,
                                                         Ptr<void>(flag_buf), 32, Ptr<void>(wide_buf), st)));
            vals.data = Ptr<void>(wide_buf);
            ftype = ARX_NUM_FLOAT64;
          }
          ARROW_ASSIGN_OR_RAISE(auto fseen, ZeroedDevice<uint32_t>(g, st));
          ARROW_ASSIGN_OR_RAISE(auto fsums, ZeroedDevice<int64_t>(g, st));     // (zero bits = 0.0)
          ARROW_ASSIGN_OR_RAISE(auto fcounts, ZeroedDevice<int64_t>(g, st));
          const size_t fws_bytes = arx_hash_sum_float_workspace_bytes(n);
          ARROW_ASSIGN_OR_RAISE(auto fws, AllocDevice(static_cast<int64_t>(fws_bytes) + 256));
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_sum_float_consume(&vals, ftype, 0, 0.0, ids, n, Ptr<void>(fws), fws_bytes + 256,
                                                                 Ptr<double>(fsums), Ptr<int64_t>(fcounts), Ptr<uint32_t>(fseen), st)));
          // pass 2: the sums of (x - mean)^k, k = 2 and — skew: 3, kurtosis: 4 — in row order like every float sum here
          ARROW_ASSIGN_OR_RAISE(auto dev_buf, AllocDevice(std::max<int64_t>(n, 1) * 8));
          std::shared_ptr<Buffer> moment[5];
          for (int power = 2; power <= 4; ++power) {
            if (power == 3 && a.kind != kSkew) continue;
            if (power == 4 && a.kind != kKurtosis) continue;
            ARROW_RETURN_NOT_OK(FromArx(arx_group_central_power(&vals, ftype, ids, n, Ptr<double>(fsums), Ptr<int64_t>(fcounts), power,
                                                                Ptr<double>(dev_buf), st)));
            ArxSpan dv = vals;
            dv.data = Ptr<void>(dev_buf);
            ARROW_ASSIGN_OR_RAISE(moment[power], ZeroedDevice<int64_t>(g, st));
            ARROW_ASSIGN_OR_RAISE(auto mcounts, ZeroedDevice<int64_t>(g, st));
            ARROW_ASSIGN_OR_RAISE(auto mseen, ZeroedDevice<uint32_t>(g, st));
            ARROW_RETURN_NOT_OK(FromArx(arx_hash_sum_float_consume(&dv, ARX_NUM_FLOAT64, 0, 0.0, ids, n, Ptr<void>(fws), fws_bytes + 256,
                                                                   Ptr<double>(moment[power]), Ptr<int64_t>(mcounts), Ptr<uint32_t>(mseen), st)));
          }
          const int stat = a.kind == kVariance ? ARX_STAT_VARIANCE : a.kind == kStddev ? ARX_STAT_STDDEV
                           : a.kind == kSkew   ? ARX_STAT_SKEW : ARX_STAT_KURTOSIS;
          ARROW_ASSIGN_OR_RAISE(auto fcol, AllocDevice(std::max<int64_t>(g, 1) * 8));
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_moments_finalize(Ptr<int64_t>(fcounts), Ptr<double>(moment[2]),
                                                                moment[3] != nullptr ? Ptr<double>(moment[3]) : nullptr,
                                                                moment[4] != nullptr ? Ptr<double>(moment[4]) : nullptr, g, stat, a.ddof,
                                                                a.biased ? 1 : 0, Ptr<double>(fcol), st)));
          // Finalize (:747-775): a value where count > ddof (unbiased skew: count > 2, kurtosis: count > 3) and count >= min_count
          const uint32_t defined_from = (a.kind == kVariance || a.kind == kStddev) ? static_cast<uint32_t>(a.ddof) + 1u
                                        : a.biased ? 1u : a.kind == kSkew ? 3u : 4u;
          HIP_RETURN_NOT_OK(hipMemsetAsync(Ptr<void>(flag_buf), 0, 32, st));
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_sum_i64_finalize(Ptr<int64_t>(fcounts), Ptr<uint32_t>(fseen), g, a.options.skip_nulls ? 1 : 0,
                                                                std::max(a.options.min_count, defined_from), Ptr<void>(bits_buf),
                                                                Ptr<int64_t>(flag_buf), st)));
          ARROW_ASSIGN_OR_RAISE(out, ToHostColumn(arrow::float64(), Ptr<void>(fcol), 8, Ptr<void>(bits_buf), g, st));
          continue;
        }
        if (NumIsFloat(a.num_type) && (a.kind == kSum || a.kind == kMean)) {
          // float32 / float64 sums and means: a double per group fed in ROW order, as the reference's accumulators are
          // (arx_hash_sum_float_consume: stable sort by group id, one walker per group)
          ARROW_ASSIGN_OR_RAISE(auto fseen, ZeroedDevice<uint32_t>(g, st));
          ARROW_ASSIGN_OR_RAISE(auto fsums, ZeroedDevice<int64_t>(g, st));     // (zero bits = 0.0)
          ARROW_ASSIGN_OR_RAISE(auto fcounts, ZeroedDevice<int64_t>(g, st));
          const size_t fws_bytes = arx_hash_sum_float_workspace_bytes(n);
          ARROW_ASSIGN_OR_RAISE(auto fws, AllocDevice(static_cast<int64_t>(fws_bytes) + 256));
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_sum_float_consume(&vals, a.num_type, 0, 0.0, ids, n, Ptr<void>(fws), fws_bytes + 256,
                                                                 Ptr<double>(fsums), Ptr<int64_t>(fcounts), Ptr<uint32_t>(fseen), st)));
          std::shared_ptr<Buffer> fcol = fsums;
          if (a.kind == kMean) {
            ARROW_ASSIGN_OR_RAISE(fcol, AllocDevice(std::max<int64_t>(g, 1) * 8));
            ARROW_RETURN_NOT_OK(FromArx(arx_hash_mean_f64_finalize(Ptr<double>(fsums), Ptr<int64_t>(fcounts), g, Ptr<double>(fcol), st)));
          }
          HIP_RETURN_NOT_OK(hipMemsetAsync(Ptr<void>(flag_buf), 0, 32, st));
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_sum_i64_finalize(Ptr<int64_t>(fcounts), Ptr<uint32_t>(fseen), g, a.options.skip_nulls ? 1 : 0,
                                                                a.options.min_count, Ptr<void>(bits_buf), Ptr<int64_t>(flag_buf), st)));
          ARROW_ASSIGN_OR_RAISE(out, ToHostColumn(arrow::float64(), Ptr<void>(fcol), 8, Ptr<void>(bits_buf), g, st));
          continue;
        }
        if (NumIsFloat(a.num_type)) {
          // float32 / float64 extrema: read as they are, folded as order keys (arx_hash_minmax_float_*)
          const auto ftype = a.out_type;
          ARROW_ASSIGN_OR_RAISE(auto fseen, ZeroedDevice<uint32_t>(g, st));
          ARROW_ASSIGN_OR_RAISE(auto fmins, AllocDevice(std::max<int64_t>(g, 1) * 8));
          ARROW_ASSIGN_OR_RAISE(auto fmaxs, AllocDevice(std::max<int64_t>(g, 1) * 8));
          ARROW_ASSIGN_OR_RAISE(auto fout, AllocDevice(std::max<int64_t>(g, 1) * 8));
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_minmax_i64_fill(Ptr<int64_t>(fmins), Ptr<int64_t>(fmaxs), 0, g, st)));
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_minmax_float_consume(&vals, a.num_type, 0, 0.0, ids, n, Ptr<int64_t>(fmins),
                                                                    Ptr<int64_t>(fmaxs), Ptr<uint32_t>(fseen), st)));
          HIP_RETURN_NOT_OK(hipMemsetAsync(Ptr<void>(flag_buf), 0, 32, st));
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_minmax_float_finalize(
              Ptr<int64_t>(fmins), Ptr<int64_t>(fmaxs), Ptr<uint32_t>(fseen), g, a.options.skip_nulls ? 1 : 0, a.num_type,
              a.kind == kMin ? Ptr<void>(fout) : nullptr, a.kind == kMax ? Ptr<void>(fout) : nullptr, Ptr<void>(bits_buf),
              Ptr<int64_t>(flag_buf), st)));
          ARROW_ASSIGN_OR_RAISE(out, ToHostColumn(ftype, Ptr<void>(fout), NumWidth(a.num_type), Ptr<void>(bits_buf), g, st));
          continue;
        }
        if (a.num_type != ARX_NUM_INT64 && a.num_type != ARX_NUM_UINT64) {   // int8 .. uint32: sign- / zero-extended once
          ARROW_ASSIGN_OR_RAISE(wide_buf, AllocDevice(std::max<int64_t>(n, 1) * 8));
          ARROW_RETURN_NOT_OK(FromArx(arx_cast_numeric(&vals, a.num_type, SumNumUnsigned(a.num_type) ? ARX_NUM_UINT64 : ARX_NUM_INT64,
                                                       /*allow_int_overflow=*/1, /*allow_float_truncate=*/1, Ptr<void>(flag_buf), 32,
                                                       Ptr<void>(wide_buf), st)));
          vals.data = Ptr<void>(wide_buf);
        }
        const auto out_field_type = a.out_type;
        std::shared_ptr<Buffer> sums, counts, seen, mins, maxs;
        ARROW_ASSIGN_OR_RAISE(seen, ZeroedDevice<uint32_t>(g, st));
        if (a.kind == kSum || a.kind == kMean) {
          ARROW_ASSIGN_OR_RAISE(sums, ZeroedDevice<int64_t>(g, st));
          ARROW_ASSIGN_OR_RAISE(counts, ZeroedDevice<int64_t>(g, st));
          const size_t ws_bytes = arx_hash_sum_consume_workspace_bytes(n, g);
          AlignedDevice ws_buf{nullptr, nullptr};
          void* ws = nullptr;
          if (ws_bytes > 0) {
            ARROW_ASSIGN_OR_RAISE(ws_buf, AllocAligned(static_cast<int64_t>(ws_bytes)));
            ws = ws_buf.ptr;
          }
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_sum_i64_consume_ws(&vals, 0, 0, ids, n, g, Ptr<int64_t>(sums), Ptr<int64_t>(counts),
                                                                  Ptr<uint32_t>(seen), ws, ws_bytes, st)));
          HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (the workspace goes back to the pool)
        }
        if (a.kind != kSum) {
          std::shared_ptr<Buffer> flip_buf;
          if (a.num_type == ARX_NUM_UINT64) {   // extrema of uint64: on x + 2^63 (mod 2^64) read as int64
            ARROW_ASSIGN_OR_RAISE(flip_buf, AllocDevice(std::max<int64_t>(n, 1) * 8));
            ARROW_RETURN_NOT_OK(FromArx(arx_arith_numeric(ARX_ARITH_ADD, 0, ARX_NUM_UINT64, vals.data, nullptr, nullptr, 0, nullptr,
                                                          &kUInt64Half, nullptr, 0, n, Ptr<void>(flip_buf), nullptr, st)));
            vals.data = Ptr<void>(flip_buf);
          }
          ARROW_ASSIGN_OR_RAISE(mins, AllocDevice(std::max<int64_t>(g, 1) * 8));
          ARROW_ASSIGN_OR_RAISE(maxs, AllocDevice(std::max<int64_t>(g, 1) * 8));
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_minmax_i64_fill(Ptr<int64_t>(mins), Ptr<int64_t>(maxs), 0, g, st)));
          std::shared_ptr<Buffer> mm_seen = seen;
          if (a.kind == kMean) {   // (the sum consume owns `seen`)
            ARROW_ASSIGN_OR_RAISE(mm_seen, ZeroedDevice<uint32_t>(g, st));
          }
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_minmax_i64_consume(&vals, 0, 0, ids, n, Ptr<int64_t>(mins), Ptr<int64_t>(maxs),
                                                                  Ptr<uint32_t>(mm_seen), st)));
          HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
        }
        HIP_RETURN_NOT_OK(hipMemsetAsync(Ptr<void>(flag_buf), 0, 32, st));
        if (a.kind == kSum) {
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_sum_i64_finalize(Ptr<int64_t>(counts), Ptr<uint32_t>(seen), g, a.options.skip_nulls ? 1 : 0,
                                                                a.options.min_count, Ptr<void>(bits_buf), Ptr<int64_t>(flag_buf), st)));
          ARROW_ASSIGN_OR_RAISE(out, ToHostColumn(out_field_type, Ptr<void>(sums), 8, Ptr<void>(bits_buf), g, st));
        } else if (a.kind == kMin || a.kind == kMax) {
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_minmax_i64_finalize(Ptr<int64_t>(mins), Ptr<int64_t>(maxs), Ptr<uint32_t>(seen), g,
                                                                   a.options.skip_nulls ? 1 : 0, Ptr<void>(bits_buf), Ptr<int64_t>(flag_buf), st)));
          std::shared_ptr<Buffer> extrema = a.kind == kMin ? mins : maxs;
          int width = 8;
          if (a.num_type == ARX_NUM_UINT64) {   // (kept as x + 2^63: the same addition maps them back)
            ARROW_ASSIGN_OR_RAISE(auto back, AllocDevice(std::max<int64_t>(g, 1) * 8));
            ARROW_RETURN_NOT_OK(FromArx(arx_arith_numeric(ARX_ARITH_ADD, 0, ARX_NUM_UINT64, Ptr<void>(extrema), nullptr, nullptr, 0, nullptr,
                                                          &kUInt64Half, nullptr, 0, g, Ptr<void>(back), nullptr, st)));
            extrema = back;
          } else if (a.num_type != ARX_NUM_INT64) {   // back to the column's own type
            width = SumNumWidth(a.num_type);
            ARROW_ASSIGN_OR_RAISE(auto narrow, AllocDevice(std::max<int64_t>(g, 1) * width));
            const ArxSpan wide{nullptr, Ptr<void>(extrema), 0, g, 0};
            ARROW_RETURN_NOT_OK(FromArx(arx_cast_numeric(&wide, ARX_NUM_INT64, a.num_type, 1, 1, Ptr<uint8_t>(flag_buf) + 16, 8,
                                                         Ptr<void>(narrow), st)));
            extrema = narrow;
          }
          ARROW_ASSIGN_OR_RAISE(out, ToHostColumn(out_field_type, Ptr<void>(extrema), width, Ptr<void>(bits_buf), g, st));
        } else {
          // hash_mean: exact while every partial sum stays below 2^53 (see plugin/hash_aggregate_more.inc)
          std::vector<int64_t> mn(g), mx(g);
          HIP_RETURN_NOT_OK(hipMemcpyAsync(mn.data(), Ptr<void>(mins), static_cast<size_t>(g) * 8, hipMemcpyDeviceToHost, st));
          HIP_RETURN_NOT_OK(hipMemcpyAsync(mx.data(), Ptr<void>(maxs), static_cast<size_t>(g) * 8, hipMemcpyDeviceToHost, st));
          HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
          uint64_t bound = 0;
          for (int64_t i = 0; i < g; ++i) {
            if (mn[i] > mx[i]) continue;
            if (a.num_type == ARX_NUM_UINT64) {
              bound = std::max(bound, static_cast<uint64_t>(mx[i]) ^ kUInt64Half);
              continue;
            }
            const uint64_t lo = mn[i] < 0 ? (0 - static_cast<uint64_t>(mn[i])) : static_cast<uint64_t>(mn[i]);
            const uint64_t hi = mx[i] < 0 ? (0 - static_cast<uint64_t>(mx[i])) : static_cast<uint64_t>(mx[i]);
            bound = std::max(bound, std::max(lo, hi));
          }
          ARROW_ASSIGN_OR_RAISE(auto means, AllocDevice(std::max<int64_t>(g, 1) * 8));
          uint32_t* d_inexact = reinterpret_cast<uint32_t*>(Ptr<uint8_t>(flag_buf) + 8);
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_mean_i64_finalize(Ptr<int64_t>(sums), Ptr<int64_t>(counts), g, bound, Ptr<double>(means), d_inexact, st)));
          ARROW_RETURN_NOT_OK(FromArx(arx_hash_sum_i64_finalize(Ptr<int64_t>(counts), Ptr<uint32_t>(seen), g, a.options.skip_nulls ? 1 : 0,
                                                                a.options.min_count, Ptr<void>(bits_buf), Ptr<int64_t>(flag_buf), st)));
          uint32_t inexact = 0;
          HIP_RETURN_NOT_OK(hipMemcpyAsync(&inexact, d_inexact, 4, hipMemcpyDeviceToHost, st));
          HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
          if (inexact != 0) {
            return Status::NotImplemented("aggregate_rocm: hash_mean(int64): a group's partial sums exceed 2^53, where the "
                                          "reference's row-order double accumulation depends on the row order");
          }
          ARROW_ASSIGN_OR_RAISE(out, ToHostColumn(arrow::float64(), Ptr<void>(means), 8, Ptr<void>(bits_buf), g, st));
        }
      }
    } else {
      for (size_t c = 0; c < columns.size(); ++c) {
        const auto type = c < static_cast<size_t>(nk) ? output_schema()->field(static_cast<int>(c))->type() : aggs_[c - nk].out_type;
        ARROW_ASSIGN_OR_RAISE(auto empty, arrow::MakeEmptyArray(type));
        columns[c] = arrow::Datum(empty);
      }
    }
    // hash_min_max: its two halves leave as one struct<min, max> column
    if (columns.size() != static_cast<size_t>(output_schema()->num_fields())) {
      std::vector<arrow::Datum> joined(columns.begin(), columns.begin() + nk);
      for (size_t ai = 0; ai < aggs_.size(); ++ai) {
        if (aggs_[ai].pair == 1 && ai + 1 < aggs_.size()) {
          const auto& vt = aggs_[ai].out_type;
          joined.push_back(arrow::Datum(ArrayData::Make(arrow::struct_({arrow::field("min", vt), arrow::field("max", vt)}), g, {nullptr},
                                                        {columns[nk + ai].array(), columns[nk + ai + 1].array()}, 0)));
          ++ai;
        } else {
          joined.push_back(columns[nk + ai]);
        }
      }
      columns = std::move(joined);
    }
    return EmitResult(this, output_, std::move(columns), g, /*any_device=*/false, st);   // (every column was made on the host)
  }

  const std::vector<int> key_cols_, key_widths_;
  const std::vector<Agg> aggs_;
  int64_t rows_ = 0;
};

// aggregate_rocm: the fused int32 -> int64 operator where it applies, the Grouper-based node for everything else
arrow::Result<ac::ExecNode*> MakeAggregateRocm(ac::ExecPlan* plan, std::vector<ac::ExecNode*> inputs,
                                               const ac::ExecNodeOptions& options) {
  if (inputs.size() != 1) return Status::Invalid("aggregate_rocm takes exactly one input");
  const auto* opts = dynamic_cast<const ac::AggregateNodeOptions*>(&options);
  if (opts == nullptr) return Status::TypeError("aggregate_rocm expects AggregateNodeOptions");
  auto fused = RocmGroupBySumNode::Make(plan, inputs, options);
  if (fused.ok() || !fused.status().IsNotImplemented()) return fused;
  auto general = RocmGroupByGeneralNode::Make(plan, inputs, *opts);
  if (general.ok() || !general.status().IsNotImplemented()) return general;
  return Status::NotImplemented(general.status().message(), " (the fused int32 -> int64 operator: ", fused.status().message(), ")");
}

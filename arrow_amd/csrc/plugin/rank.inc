// rank / rank_quantile / select_k_unstable / partition_nth_indices on device-resident data (round 6, §8 f3).
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous namespace.
//
// The reference's functions are MetaFunctions over its CPU array sorters (RankMetaFunctionBase::Rank,
// kernels/vector_rank.cc:386-420; SelectKUnstableMetaFunction, kernels/vector_select_k.cc:640-740) and, for
// partition_nth_indices, a vector kernel around std::nth_element (kernels/vector_array_sort.cc:56-95): all of them read
// the values through host pointers.  The wrappers registered here under the same names take device-resident arrays
// (kROCM buffers) through the registered array_sort_indices — the HIP sort — and, for the ranks, arx_rank (csrc/rank.hip)
// over its output; everything else (host data, types without a device sort) goes to the stock function untouched.
//   * rank: sort + MarkDuplicates + the tiebreaker's walk; uint64 ranks in HBM.  rank_quantile: the same walk, float64.
//   * select_k_unstable: the first k rows of the sort order under the key's order / null placement (arrays, chunked
//     arrays) or of the multi-key chain (record batches, tables).  "Unstable" promises nothing about ties; the stable
//     sort's order is one valid answer.
//   * partition_nth_indices: any permutation with the pivot-th smallest in place is valid; the full sort is one.

bool DatumOnRocm(const arrow::Datum& d) {
  switch (d.kind()) {
    case arrow::Datum::ARRAY: return DataOnRocm(*d.array());
    case arrow::Datum::CHUNKED_ARRAY:
      for (const auto& chunk : d.chunked_array()->chunks()) {
        if (DataOnRocm(*chunk->data())) return true;
      }
      return false;
    case arrow::Datum::RECORD_BATCH:
      for (int i = 0; i < d.record_batch()->num_columns(); ++i) {
        if (DataOnRocm(*d.record_batch()->column_data(i))) return true;
      }
      return false;
    case arrow::Datum::TABLE:
      for (int i = 0; i < d.table()->num_columns(); ++i) {
        for (const auto& chunk : d.table()->column(i)->chunks()) {
          if (DataOnRocm(*chunk->data())) return true;
        }
      }
      return false;
    default: return false;
  }
}

// a device-resident array or chunked array as ONE array (chunks concatenated in HBM, as the sort wrapper does)
arrow::Result<std::shared_ptr<ArrayData>> OneDeviceArray(const arrow::Datum& d) {
  if (d.is_array()) return d.array();
  const auto& c = *d.chunked_array();
  if (c.num_chunks() == 1) return c.chunk(0)->data();
  if (c.num_chunks() == 0) return ArrayData::Make(c.type(), 0, {nullptr, nullptr}, 0);
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  std::vector<std::shared_ptr<ArrayData>> chunks;
  for (const auto& chunk : c.chunks()) chunks.push_back(chunk->data());
  ARROW_ASSIGN_OR_RAISE(auto whole, ConcatOnDevice(c.type(), chunks, st));
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  return whole;
}

// ARX_KEY_* of a type the ranks are computed for on the device (the physical integer of the temporal types), -1: none
int RankKeyType(const arrow::DataType& type) {
  switch (type.id()) {
    case Type::UINT64: return ARX_KEY_UINT64;
    case Type::INT64: case Type::DATE64: case Type::TIMESTAMP: case Type::DURATION: case Type::TIME64: return ARX_KEY_INT64;
    case Type::UINT32: return ARX_KEY_UINT32;
    case Type::INT32: case Type::DATE32: case Type::TIME32: return ARX_KEY_INT32;
    case Type::DOUBLE: return ARX_KEY_FLOAT64;
    case Type::FLOAT: return ARX_KEY_FLOAT32;
    default: return -1;
  }
}

// RankMetaFunctionBase::Rank for a device-resident array: tiebreaker = ARX_RANK_*
arrow::Result<arrow::Datum> RankOnDevice(const arrow::Datum& input, cp::SortOrder order, cp::NullPlacement placement, int tiebreaker,
                                         cp::ExecContext* ctx) {
  ARROW_ASSIGN_OR_RAISE(auto values, OneDeviceArray(input));
  const int key_type = RankKeyType(*values->type);
  const auto out_type = tiebreaker >= ARX_RANK_QUANTILE ? arrow::float64() : arrow::uint64();
  if (key_type < 0) {
    return Status::NotImplemented("arrow_amd: rank of device-resident ", values->type->ToString(), " values");
  }
  const int64_t n = values->length;
  if (n == 0) return arrow::Datum(ArrayData::Make(out_type, 0, {nullptr, nullptr}, 0));
  const cp::ArraySortOptions sort_options(order, placement);
  ARROW_ASSIGN_OR_RAISE(arrow::Datum perm, cp::CallFunction("array_sort_indices", {arrow::Datum(values)}, &sort_options, ctx));
  if (!DataOnRocm(*perm.array())) return Status::Invalid("arrow_amd: the sort of a device array left the device");
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  ArxSpan dv{};
  ARROW_RETURN_NOT_OK(DeviceSpan(ArraySpan(*values), &dv));
  ARROW_ASSIGN_OR_RAISE(std::shared_ptr<Buffer> out, AllocDevice(n * 8));
  void* ws = nullptr;
  const size_t ws_bytes = arx_rank_workspace_bytes(n);
  ARROW_RETURN_NOT_OK(t_scratch.Get(kWs, ws_bytes + 256, &ws));
  ws = Align256(ws);
  const auto* rows = reinterpret_cast<const uint64_t*>(perm.array()->buffers[1]->address()) + perm.array()->offset;
  ARROW_RETURN_NOT_OK(FromArx(arx_rank(&dv, key_type, rows, tiebreaker, ws, ws_bytes, reinterpret_cast<void*>(out->mutable_address()), st)));
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  CountGpu(kFnSort);
  return arrow::Datum(ArrayData::Make(out_type, n, {nullptr, std::move(out)}, 0));
}

template <typename Options>
void ResolveRankOrder(const Options& options, cp::SortOrder* order, cp::NullPlacement* placement) {
  // (RankMetaFunctionBase::Rank, vector_rank.cc:392-402: the first sort key, the deprecated option-wide placement on top)
  *order = cp::SortOrder::Ascending;
  *placement = cp::NullPlacement::AtEnd;
  const auto keys = options.GetSortKeys();
  if (!keys.empty()) {
    *order = keys[0].order;
    *placement = keys[0].null_placement;
  }
}

class RocmRankMetaFunction : public cp::MetaFunction {
 public:
  // quantile: 0 = "rank" (RankOptions), ARX_RANK_QUANTILE / ARX_RANK_NORMAL = "rank_quantile" / "rank_normal" (RankQuantileOptions)
  RocmRankMetaFunction(std::string name, std::shared_ptr<cp::Function> stock, int quantile)
      : cp::MetaFunction(std::move(name), cp::Arity::Unary(), stock->doc(), stock->default_options()),
        stock_(std::move(stock)), quantile_(quantile) {}

  arrow::Result<arrow::Datum> ExecuteImpl(const std::vector<arrow::Datum>& args, const cp::FunctionOptions* options,
                                          cp::ExecContext* ctx) const override {
    if (args.size() != 1 || options == nullptr || !(args[0].is_array() || args[0].is_chunked_array()) || !DatumOnRocm(args[0])) {
      return stock_->Execute(args, options, ctx);
    }
    cp::SortOrder order;
    cp::NullPlacement placement;
    int tiebreaker = quantile_;
    if (quantile_ != 0) {
      ResolveRankOrder(*static_cast<const cp::RankQuantileOptions*>(options), &order, &placement);
    } else {
      const auto& rank_options = *static_cast<const cp::RankOptions*>(options);
      ResolveRankOrder(rank_options, &order, &placement);
      switch (rank_options.tiebreaker) {
        case cp::RankOptions::Min: tiebreaker = ARX_RANK_MIN; break;
        case cp::RankOptions::Max: tiebreaker = ARX_RANK_MAX; break;
        case cp::RankOptions::First: tiebreaker = ARX_RANK_FIRST; break;
        default: tiebreaker = ARX_RANK_DENSE; break;
      }
    }
    return RankOnDevice(args[0], order, placement, tiebreaker, ctx);
  }

 private:
  std::shared_ptr<cp::Function> stock_;
  const int quantile_;
};

// select_k by a THRESHOLD instead of a sort (round 6; the mirror's compute._select_k_by_threshold): uint64 / int64 (and the
// 64-bit temporal) keys, k much smaller than the column, every selected row a non-null.  One pass for a 4096-bin histogram of
// the keys over their sampled, widened range (arx_sort_key_range_sampled + arx_sort_key_histogram_window: what the sharded
// sort places its splitters with), the bin in which the k-th smallest key falls, ONE comparison of the column against that
// bin's upper edge (less_equal / greater_equal), indices_nonzero of the bitmap (the candidates' rows, ascending), and the sort
// of the candidates' keys alone: the candidates are exactly the rows whose bin is at most that bin (monotone in the key,
// keys outside the sampled range saturate into the end bins), they come in row order and the sort is stable — index for
// index the head of the full stable sort.  *done == false: not this case.
Status SelectKByThreshold(const std::shared_ptr<ArrayData>& values, int64_t k, cp::SortOrder order, cp::NullPlacement placement,
                          cp::ExecContext* ctx, bool* done, arrow::Datum* out) {
  *done = false;
  const int64_t n = values->length;
  const int key_type = RankKeyType(*values->type);
  if ((key_type != ARX_KEY_UINT64 && key_type != ARX_KEY_INT64) || n < g_select_k_min_rows.load() || n > 0xFFFFFFFFll || k <= 0 || k * 16 > n) {
    return Status::OK();
  }
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  ArxSpan dv{};
  ARROW_RETURN_NOT_OK(DeviceSpan(ArraySpan(*values), &dv));
  int64_t nulls = 0;
  if (dv.validity != nullptr) {
    if (placement == cp::NullPlacement::AtStart) return Status::OK();
    void* cws = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(kCounter, 64, &cws));
    int64_t set_bits = 0;
    ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_popcount(dv.validity, dv.offset, n, cws, 64, &set_bits, st)));
    nulls = n - set_bits;
    if (k > n - nulls) return Status::OK();
  }
  const int is_signed = key_type == ARX_KEY_INT64 ? 1 : 0;
  const int order_code = order == cp::SortOrder::Descending ? ARX_SORT_DESCENDING : ARX_SORT_ASCENDING;
  ARROW_ASSIGN_OR_RAISE(auto d_range, AllocDevice(16));
  HIP_RETURN_NOT_OK(hipMemsetAsync(reinterpret_cast<void*>(d_range->mutable_address()), 0, 16, st));
  ARROW_RETURN_NOT_OK(FromArx(arx_sort_key_range_sampled(&dv, is_signed, order_code, 4, reinterpret_cast<uint64_t*>(d_range->mutable_address()), st)));
  uint64_t range[2];
  HIP_RETURN_NOT_OK(hipMemcpyAsync(range, reinterpret_cast<const void*>(d_range->address()), 16, hipMemcpyDeviceToHost, st));
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  uint64_t key_min = ~range[0], key_max = range[1];
  if (key_max <= key_min) return Status::OK();
  const uint64_t margin = ((key_max - key_min) >> 6) + 1;
  key_min = key_min > margin ? key_min - margin : 0;
  key_max = key_max < ~uint64_t(0) - margin ? key_max + margin : ~uint64_t(0);
  ArxSortKeyWindow window{key_min, __builtin_clzll(key_max - key_min), 0};
  constexpr int kBits = 12;
  ARROW_ASSIGN_OR_RAISE(auto d_hist, AllocDevice((1 << kBits) * 8));
  HIP_RETURN_NOT_OK(hipMemsetAsync(reinterpret_cast<void*>(d_hist->mutable_address()), 0, (1 << kBits) * 8, st));
  ARROW_RETURN_NOT_OK(FromArx(arx_sort_key_histogram_window(&dv, is_signed, order_code, kBits, &window,
                                                            reinterpret_cast<uint64_t*>(d_hist->mutable_address()), st)));
  std::vector<uint64_t> hist(1 << kBits);
  HIP_RETURN_NOT_OK(hipMemcpyAsync(hist.data(), reinterpret_cast<const void*>(d_hist->address()), hist.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  int b = 0;
  uint64_t below = 0;
  for (; b < (1 << kBits); ++b) {
    below += hist[b];
    if (below >= static_cast<uint64_t>(k)) break;
  }
  if (b >= (1 << kBits) - 1 || below * 4 > static_cast<uint64_t>(n)) return Status::OK();   // the open last bin, or a bin with a fifth of the column
  const unsigned __int128 top = ((static_cast<unsigned __int128>(b) + 1) << (64 - kBits)) - 1;
  const uint64_t reach = static_cast<uint64_t>(top >> window.shift);
  if (reach >= ~uint64_t(0) - key_min) return Status::OK();
  uint64_t raw = key_min + reach;   // the largest order-transformed key whose bin is at most b -> the column's value
  if (order == cp::SortOrder::Descending) raw = ~raw;
  if (is_signed) raw ^= uint64_t(1) << 63;
  // the bound as a scalar of the column's own type (temporal types compare through their physical integer)
  std::shared_ptr<arrow::Scalar> bound;
  auto physical = values->Copy();
  if (is_signed) {
    physical->type = arrow::int64();
    bound = std::make_shared<arrow::Int64Scalar>(static_cast<int64_t>(raw));
  } else {
    bound = std::make_shared<arrow::UInt64Scalar>(raw);
  }
  ARROW_ASSIGN_OR_RAISE(arrow::Datum mask, cp::CallFunction(order == cp::SortOrder::Descending ? "greater_equal" : "less_equal",
                                                            {arrow::Datum(physical), arrow::Datum(bound)}, ctx));
  ARROW_ASSIGN_OR_RAISE(arrow::Datum rows, cp::CallFunction("indices_nonzero", {mask}, ctx));
  if (rows.length() != static_cast<int64_t>(below)) {
    return Status::Invalid("arrow_amd select_k: ", rows.length(), " candidates, the histogram promised ", below);
  }
  const cp::TakeOptions no_check = cp::TakeOptions::NoBoundsCheck();
  ARROW_ASSIGN_OR_RAISE(arrow::Datum cand, cp::CallFunction("array_take", {arrow::Datum(physical), rows}, &no_check, ctx));
  const cp::ArraySortOptions sort_options(order, cp::NullPlacement::AtEnd);
  ARROW_ASSIGN_OR_RAISE(arrow::Datum perm, cp::CallFunction("array_sort_indices", {cand}, &sort_options, ctx));
  ARROW_ASSIGN_OR_RAISE(*out, cp::CallFunction("array_take", {rows, arrow::Datum(perm.array()->Slice(0, k))}, &no_check, ctx));
  g_select_k_threshold_runs.fetch_add(1);
  *done = true;
  return Status::OK();
}

// select_k_unstable: SelectKUnstableMetaFunction (vector_select_k.cc:640-740) — k checked as there, then the head of the
// device sort's order
class RocmSelectKMetaFunction : public cp::MetaFunction {
 public:
  explicit RocmSelectKMetaFunction(std::shared_ptr<cp::Function> stock)
      : cp::MetaFunction("select_k_unstable", cp::Arity::Unary(), stock->doc(), stock->default_options()),
        stock_(std::move(stock)) {}

  arrow::Result<arrow::Datum> ExecuteImpl(const std::vector<arrow::Datum>& args, const cp::FunctionOptions* options,
                                          cp::ExecContext* ctx) const override {
    if (args.size() != 1 || options == nullptr || !DatumOnRocm(args[0])) return stock_->Execute(args, options, ctx);
    const auto& select_options = *static_cast<const cp::SelectKOptions*>(options);
    if (select_options.k < 0) {
      return Status::Invalid("select_k_unstable requires a nonnegative `k`, got ", select_options.k);
    }
    const std::vector<cp::SortKey> sort_keys = select_options.GetSortKeys();
    if (sort_keys.empty()) return Status::Invalid("select_k_unstable requires a non-empty `sort_keys`");
    arrow::Datum perm;
    if (args[0].is_array() || args[0].is_chunked_array()) {
      if (sort_keys.size() != 1) {
        return Status::Invalid("select_k_unstable: exactly one sort key for an array");   // (the reference's array selectors take the first)
      }
      ARROW_ASSIGN_OR_RAISE(auto values, OneDeviceArray(args[0]));
      if (values->length == 0) return arrow::Datum(ArrayData::Make(arrow::uint64(), 0, {nullptr, nullptr}, 0));
      bool by_threshold = false;
      arrow::Datum picked;
      ARROW_RETURN_NOT_OK(SelectKByThreshold(values, select_options.k, sort_keys[0].order, sort_keys[0].null_placement, ctx, &by_threshold, &picked));
      if (by_threshold) return picked;
      const cp::ArraySortOptions sort_options(sort_keys[0].order, sort_keys[0].null_placement);
      ARROW_ASSIGN_OR_RAISE(perm, cp::CallFunction("array_sort_indices", {arrow::Datum(values)}, &sort_options, ctx));
    } else {
      const cp::SortOptions sort_options(sort_keys);
      ARROW_ASSIGN_OR_RAISE(perm, cp::CallFunction("sort_indices", {args[0]}, &sort_options, ctx));
    }
    const int64_t k = std::min<int64_t>(select_options.k, perm.length());
    return arrow::Datum(perm.array()->Slice(0, k));
  }

 private:
  std::shared_ptr<cp::Function> stock_;
};

// partition_nth_indices: PartitionNthToIndices::Exec (vector_array_sort.cc:56-95) — the pivot checked as there
class RocmPartitionNthMetaFunction : public cp::MetaFunction {
 public:
  explicit RocmPartitionNthMetaFunction(std::shared_ptr<cp::Function> stock)
      : cp::MetaFunction("partition_nth_indices", cp::Arity::Unary(), stock->doc(), stock->default_options()),
        stock_(std::move(stock)) {}

  arrow::Result<arrow::Datum> ExecuteImpl(const std::vector<arrow::Datum>& args, const cp::FunctionOptions* options,
                                          cp::ExecContext* ctx) const override {
    if (args.size() != 1 || !args[0].is_array() || !DatumOnRocm(args[0])) return stock_->Execute(args, options, ctx);
    if (options == nullptr) return Status::Invalid("NthToIndices requires PartitionNthOptions");
    const auto& nth_options = *static_cast<const cp::PartitionNthOptions*>(options);
    if (nth_options.pivot > args[0].length()) return Status::IndexError("NthToIndices index out of bound");
    const cp::ArraySortOptions sort_options(cp::SortOrder::Ascending, nth_options.null_placement);
    return cp::CallFunction("array_sort_indices", {args[0]}, &sort_options, ctx);
  }

 private:
  std::shared_ptr<cp::Function> stock_;
};

Status RegisterRankFunctions(cp::FunctionRegistry* reg) {
  for (const char* name : {"rank", "rank_quantile", "rank_normal"}) {
    ARROW_ASSIGN_OR_RAISE(auto stock, reg->GetFunction(name));
    const int quantile = std::string(name) == "rank_quantile" ? ARX_RANK_QUANTILE : std::string(name) == "rank_normal" ? ARX_RANK_NORMAL : 0;
    ARROW_RETURN_NOT_OK(reg->AddFunction(std::make_shared<RocmRankMetaFunction>(name, std::move(stock), quantile),
                                         /*allow_overwrite=*/true));
  }
  {
    ARROW_ASSIGN_OR_RAISE(auto stock, reg->GetFunction("select_k_unstable"));
    ARROW_RETURN_NOT_OK(reg->AddFunction(std::make_shared<RocmSelectKMetaFunction>(std::move(stock)), /*allow_overwrite=*/true));
  }
  {
    ARROW_ASSIGN_OR_RAISE(auto stock, reg->GetFunction("partition_nth_indices"));
    ARROW_RETURN_NOT_OK(reg->AddFunction(std::make_shared<RocmPartitionNthMetaFunction>(std::move(stock)), /*allow_overwrite=*/true));
  }
  return Status::OK();
}

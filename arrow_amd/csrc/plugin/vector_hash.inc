// unique / value_counts / dictionary_encode on device-resident arrays (the device Grouper), drop_null, indices_nonzero.
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- hash vector kernels
// The reference's hash kernels (kernels/vector_hash.cc) run a three-step protocol per call: init -> a HashKernel
// state (a memo table), exec per chunk -> Append + Flush (:603-608; dictionary_encode flushes the chunk's indices),
// finalize -> the dictionary / the counts (:610-663).  Here the memo table is the device Grouper (csrc/grouper.hip:
// one fixed-width key column, ids in order of first appearance, a null is a key of its own — exactly UniqueAction /
// ValueCountsAction / DictEncodeAction's order, :65-270), the counts are hash_count(ALL) over the ids, and
//   unique            = GetUniques
//   value_counts      = struct{GetUniques, counts}
//   dictionary_encode = ids as int32 indices + GetUniques as the dictionary; null_encoding MASK (the default) leaves
//                       the null out of the dictionary: its entry is dropped and later ids move down by one
// Values compare by their bits, like the reference's physical-type memo tables (float -0.0 / 0.0 and NaN payloads
// stay distinct).  Host arrays keep the reference kernels (a stock state beside ours, one route per call).
enum HashVectorKind { kHashUnique = 0, kHashValueCounts, kHashDictEncode };

struct DeviceHashState : public cp::KernelState {
  HashVectorKind kind = kHashUnique;
  std::unique_ptr<cp::KernelState> stock;
  bool used_stock = false, used_device = false;
  bool encode_nulls = false;                       // DictionaryEncodeOptions::ENCODE
  std::shared_ptr<arrow::DataType> type;
  int width = 0;
  std::shared_ptr<Buffer> table_buf, counts_buf;   // the Grouper state, the per-group row counts (value_counts)
  void* table = nullptr;
  int64_t max_groups = 0, num_groups = 0, counts_cap = 0;
};

StockKernel g_stock_unique, g_stock_value_counts, g_stock_dict_encode;
cp::VectorKernel::FinalizeFunc g_stock_unique_finalize = nullptr, g_stock_value_counts_finalize = nullptr,
                               g_stock_dict_encode_finalize = nullptr;

template <HashVectorKind KIND>
const StockKernel& StockHashKernel() {
  return KIND == kHashUnique ? g_stock_unique : KIND == kHashValueCounts ? g_stock_value_counts : g_stock_dict_encode;
}

// column `col` of the Grouper's unique key rows as device buffers (+ its null count)
Status HashUniques(DeviceHashState* s, hipStream_t st, std::shared_ptr<Buffer>* values, std::shared_ptr<Buffer>* validity,
                   int64_t* null_count) {
  const int64_t g = s->num_groups;
  ARROW_ASSIGN_OR_RAISE(*values, AllocDevice(std::max<int64_t>(g, 1) * s->width));
  ARROW_ASSIGN_OR_RAISE(*validity, AllocDevice(((g + 63) / 64) * 8 + 8));
  *null_count = 0;
  if (g == 0) return Status::OK();
  const int32_t w = s->width;
  return FromArx(arx_grouper_get_uniques(s->table, s->max_groups, &w, 1, 0, reinterpret_cast<void*>((*values)->mutable_address()),
                                         reinterpret_cast<uint8_t*>((*validity)->mutable_address()), null_count, st));
}

// room for `more` new groups: a larger table re-consumes the old table's uniques in id order, which hands every one of
// them its old id again (ids are the order of first appearance)
Status HashEnsureCapacity(DeviceHashState* s, int64_t more, hipStream_t st) {
  const int64_t need = s->num_groups + more + 16;
  if (s->table != nullptr && need <= s->max_groups) return Status::OK();
  const int64_t fresh_max = std::max<int64_t>({need, 2 * s->max_groups, 1 << 12});
  ARROW_ASSIGN_OR_RAISE(auto fresh_table, AllocAligned(static_cast<int64_t>(arx_grouper_state_bytes(fresh_max))));
  void* const fresh = fresh_table.ptr;
  ARROW_RETURN_NOT_OK(FromArx(arx_grouper_init(fresh, fresh_max, st)));
  if (s->table != nullptr && s->num_groups > 0) {
    std::shared_ptr<Buffer> values, validity;
    int64_t nulls = 0;
    ARROW_RETURN_NOT_OK(HashUniques(s, st, &values, &validity, &nulls));
    ArxSpan sp{reinterpret_cast<const void*>(validity->address()), reinterpret_cast<const void*>(values->address()), 0,
               s->num_groups, nulls};
    const int32_t w = s->width;
    const size_t ws_bytes = arx_grouper_consume_workspace_bytes(s->num_groups);
    void *ws = nullptr, *ids = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(kWs, ws_bytes + 256, &ws));
    ws = Align256(ws);
    ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2, static_cast<size_t>(s->num_groups) * 4 + 64, &ids));
    ARROW_RETURN_NOT_OK(FromArx(arx_grouper_consume(fresh, fresh_max, &sp, &w, 1, ws, ws_bytes, static_cast<uint32_t*>(ids), st)));
  }
  s->table_buf = std::move(fresh_table.buffer);
  s->table = fresh;
  s->max_groups = fresh_max;
  return Status::OK();
}

template <HashVectorKind KIND>
Status HashVectorExec(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  auto* s = static_cast<DeviceHashState*>(ctx->state());
  const ArraySpan& values = batch[0].array;
  if (!OnRocm(values)) {
    if (s->used_device) return Status::NotImplemented("arrow_amd: host and device-resident chunks in one hash kernel call");
    s->used_stock = true;
    return RunStock(kFnUnique, StockHashKernel<KIND>(), s->stock.get(), ctx, batch, out);
  }
  if (s->used_stock) return Status::NotImplemented("arrow_amd: host and device-resident chunks in one hash kernel call");
  if (s->width != 1 && s->width != 2 && s->width != 4 && s->width != 8) {
    return Status::NotImplemented("arrow_amd: ", KIND == kHashUnique ? "unique" : KIND == kHashValueCounts ? "value_counts" : "dictionary_encode",
                                  " of device-resident ", values.type->ToString(), " arrays");
  }
  s->used_device = true;
  const int64_t n = values.length;
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  ArrayData* out_arr = out->array_data().get();
  if (KIND == kHashDictEncode) {   // the chunk's indices (Flush): int32, validity = the values' (MASK) or none (ENCODE)
    out_arr->type = arrow::int32();
    out_arr->length = n;
    out_arr->null_count = 0;
    out_arr->buffers.assign(2, nullptr);
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice(std::max<int64_t>(n, 1) * 4));
  }
  if (n == 0) return Status::OK();
  ARROW_RETURN_NOT_OK(HashEnsureCapacity(s, n, st));
  ArxSpan sp{};
  ARROW_RETURN_NOT_OK(DeviceSpan(values, &sp));
  const int32_t w = s->width;
  const size_t ws_bytes = arx_grouper_consume_workspace_bytes(n);
  void *ws = nullptr, *ids = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kWs, ws_bytes + 256, &ws));
  ws = Align256(ws);
  if (KIND == kHashDictEncode) {
    ids = reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address());
  } else {
    ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2, static_cast<size_t>(n) * 4 + 64, &ids));
  }
  ARROW_RETURN_NOT_OK(FromArx(arx_grouper_consume(s->table, s->max_groups, &sp, &w, 1, ws, ws_bytes, static_cast<uint32_t*>(ids), st)));
  ARROW_RETURN_NOT_OK(FromArx(arx_grouper_num_groups(s->table, &s->num_groups, st)));
  if (KIND == kHashValueCounts) {
    if (s->num_groups > s->counts_cap) {
      const int64_t cap = std::max<int64_t>({s->num_groups, 2 * s->counts_cap, 1 << 12});
      ARROW_ASSIGN_OR_RAISE(auto fresh, AllocDevice(cap * 8));
      HIP_RETURN_NOT_OK(hipMemsetAsync(reinterpret_cast<void*>(fresh->mutable_address()), 0, static_cast<size_t>(cap) * 8, st));
      if (s->counts_buf != nullptr && s->counts_cap > 0) {
        HIP_RETURN_NOT_OK(hipMemcpyAsync(reinterpret_cast<void*>(fresh->mutable_address()),
                                         reinterpret_cast<const void*>(s->counts_buf->address()),
                                         static_cast<size_t>(s->counts_cap) * 8, hipMemcpyDeviceToDevice, st));
      }
      HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
      s->counts_buf = std::move(fresh);
      s->counts_cap = cap;
    }
    ARROW_RETURN_NOT_OK(FromArx(arx_hash_count_consume(nullptr, 0, 0, ARX_COUNT_ALL, static_cast<const uint32_t*>(ids), n,
                                                       reinterpret_cast<int64_t*>(s->counts_buf->mutable_address()), st)));
  }
  if (KIND == kHashDictEncode && !s->encode_nulls && sp.validity != nullptr) {
    if (values.offset == 0) {
      out_arr->buffers[0] = values.GetBuffer(0);
    } else {
      ARROW_ASSIGN_OR_RAISE(out_arr->buffers[0], AllocDevice(((n + 63) / 64) * 8));
      ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy(sp.validity, sp.offset, n,
                                                  reinterpret_cast<void*>(out_arr->buffers[0]->mutable_address()), st)));
    }
    ARROW_ASSIGN_OR_RAISE(out_arr->null_count, DeviceNullCount(*out_arr->buffers[0], n, st));
    if (out_arr->null_count == 0) out_arr->buffers[0] = nullptr;
  }
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  CountGpu(kFnUnique);
  return Status::OK();
}

// the dictionary: the Grouper's uniques; with drop_null the null's entry is left out (*null_id = its id, or -1)
arrow::Result<std::shared_ptr<ArrayData>> HashDictionary(DeviceHashState* s, bool drop_null, hipStream_t st, int64_t* null_id);

template <HashVectorKind KIND>
Status HashVectorFinalize(cp::KernelContext* ctx, std::vector<arrow::Datum>* out) {
  auto* s = static_cast<DeviceHashState*>(ctx->state());
  if (!s->used_device) {
    cp::VectorKernel::FinalizeFunc stock = KIND == kHashUnique ? g_stock_unique_finalize
                                           : KIND == kHashValueCounts ? g_stock_value_counts_finalize
                                                                      : g_stock_dict_encode_finalize;
    ctx->SetState(s->stock.get());
    Status status = stock(ctx, out);
    ctx->SetState(s);
    return status;
  }
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  int64_t null_id = -1;
  if (KIND == kHashUnique) {
    ARROW_ASSIGN_OR_RAISE(auto uniques, HashDictionary(s, false, st, &null_id));
    *out = {arrow::Datum(std::move(uniques))};
  } else if (KIND == kHashValueCounts) {
    // BoxValueCounts (vector_hash.cc): struct{values: T, counts: int64}
    ARROW_ASSIGN_OR_RAISE(auto uniques, HashDictionary(s, false, st, &null_id));
    const int64_t g = s->num_groups;
    ARROW_ASSIGN_OR_RAISE(auto counts_buf, AllocDevice(std::max<int64_t>(g, 1) * 8));
    if (g > 0) {
      ARROW_RETURN_NOT_OK(FromArx(arx_buffer_copy(reinterpret_cast<const void*>(s->counts_buf->address()),
                                                  reinterpret_cast<void*>(counts_buf->mutable_address()), g * 8, st)));
      HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    }
    auto counts = ArrayData::Make(arrow::int64(), g, {nullptr, std::move(counts_buf)}, 0);
    auto type = arrow::struct_({arrow::field("values", s->type), arrow::field("counts", arrow::int64())});
    auto boxed = ArrayData::Make(std::move(type), g, {nullptr}, {std::move(uniques), std::move(counts)}, 0);
    *out = {arrow::Datum(std::move(boxed))};
  } else {
    ARROW_ASSIGN_OR_RAISE(auto dict, HashDictionary(s, !s->encode_nulls, st, &null_id));
    auto dict_type = arrow::dictionary(arrow::int32(), s->type);
    for (auto& datum : *out) {
      std::shared_ptr<ArrayData> idx = datum.array();
      if (null_id >= 0 && idx->length > 0) {   // MASK: the ids behind the null's move down (the null rows are masked)
        ARROW_RETURN_NOT_OK(FromArx(arx_group_ids_skip_group(reinterpret_cast<uint32_t*>(idx->buffers[1]->mutable_address()),
                                                             idx->length, static_cast<uint32_t>(null_id), st)));
      }
      auto encoded = idx->Copy();
      encoded->type = dict_type;
      encoded->dictionary = dict;
      datum = arrow::Datum(std::move(encoded));
    }
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  }
  return Status::OK();
}

// ---------------------------------------------------------------- drop_null / indices_nonzero
// compaction of device values under a device bitmap used as the mask (no mask validity): the large-array branch of
// FilterExec without the Arrow plumbing
Status CompactByBitmap(const ArxSpan& dv, int width, const void* mask_bits, int64_t mask_offset, int64_t n, hipStream_t st,
                       std::shared_ptr<Buffer>* out_values, std::shared_ptr<Buffer>* out_validity, int64_t* out_length,
                       int64_t* out_null_count) {
  ArxSpan dm{nullptr, mask_bits, mask_offset, n, 0};
  const size_t ws_bytes = arx_filter_workspace_bytes(n);
  void* ws = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kWs, ws_bytes, &ws));
  int64_t out_len = 0;
  ARROW_RETURN_NOT_OK(FromArx(arx_filter_count(&dm, ARX_FILTER_DROP, ws, ws_bytes, &out_len, st)));
  ARROW_ASSIGN_OR_RAISE(*out_values, AllocDevice(std::max<int64_t>(out_len, 1) * width));
  void* d_valid = nullptr;
  *out_validity = nullptr;
  if (dv.validity != nullptr && dv.null_count != 0) {
    ARROW_ASSIGN_OR_RAISE(*out_validity, AllocDevice(((out_len + 63) / 64) * 8 + 8));
    d_valid = reinterpret_cast<void*>((*out_validity)->mutable_address());
  }
  ARROW_RETURN_NOT_OK(FromArx(arx_filter_exec(&dv, width, &dm, ARX_FILTER_DROP, ws, out_len,
                                              reinterpret_cast<void*>((*out_values)->mutable_address()), d_valid, st)));
  *out_length = out_len;
  *out_null_count = 0;
  if (d_valid != nullptr) {
    ARROW_ASSIGN_OR_RAISE(*out_null_count, DeviceNullCount(**out_validity, out_len, st));
  }
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  return Status::OK();
}

arrow::Result<std::shared_ptr<ArrayData>> HashDictionary(DeviceHashState* s, bool drop_null, hipStream_t st, int64_t* null_id) {
  std::shared_ptr<Buffer> values, validity;
  int64_t nulls = 0;
  ARROW_RETURN_NOT_OK(HashUniques(s, st, &values, &validity, &nulls));
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  const int64_t g = s->num_groups;
  *null_id = -1;
  if (nulls == 0) return ArrayData::Make(s->type, g, {nullptr, std::move(values)}, 0);
  if (!drop_null) return ArrayData::Make(s->type, g, {std::move(validity), std::move(values)}, nulls);
  // the one null entry goes: its id = the position of the clear bit (first set bit of the inverted bitmap)
  void* d_idx = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2, 256, &d_idx));
  {
    // indices of the rows the inverted validity selects: arx_boolean_invert + GetTakeIndices over g bits
    ARROW_ASSIGN_OR_RAISE(auto inv, AllocDevice(((g + 63) / 64) * 8 + 8));
    ARROW_RETURN_NOT_OK(FromArx(arx_boolean_invert(reinterpret_cast<const void*>(validity->address()), 0, g,
                                                   reinterpret_cast<void*>(inv->mutable_address()), st)));
    ArxSpan dm{nullptr, reinterpret_cast<const void*>(inv->address()), 0, g, 0};
    const size_t ws_bytes = arx_filter_workspace_bytes(g);
    void* ws = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(kWs, ws_bytes, &ws));
    int64_t cnt = 0;
    ARROW_RETURN_NOT_OK(FromArx(arx_filter_count(&dm, ARX_FILTER_DROP, ws, ws_bytes, &cnt, st)));
    if (cnt != 1) return Status::Invalid("arrow_amd: internal error (", cnt, " null entries among the unique values)");
    ARROW_RETURN_NOT_OK(FromArx(arx_mask_to_indices(&dm, ARX_FILTER_DROP, ws, cnt, 4, d_idx, nullptr, st)));
    uint32_t pos = 0;
    HIP_RETURN_NOT_OK(hipMemcpyAsync(&pos, d_idx, 4, hipMemcpyDeviceToHost, st));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    *null_id = pos;
  }
  ArxSpan dv{nullptr, reinterpret_cast<const void*>(values->address()), 0, g, 0};
  std::shared_ptr<Buffer> kept, kept_validity;
  int64_t kept_len = 0, kept_nulls = 0;
  ARROW_RETURN_NOT_OK(CompactByBitmap(dv, s->width, reinterpret_cast<const void*>(validity->address()), 0, g, st, &kept,
                                      &kept_validity, &kept_len, &kept_nulls));
  return ArrayData::Make(s->type, kept_len, {nullptr, std::move(kept)}, 0);
}

// DropNull (kernels/vector_selection.cc:71-90 DropNullArray: no nulls -> the input itself; else Filter(values,
// validity as a boolean array)) for device-resident fixed-width arrays; everything else goes to the stock function.
class RocmDropNullMetaFunction : public cp::MetaFunction {
 public:
  explicit RocmDropNullMetaFunction(std::shared_ptr<cp::Function> stock)
      : cp::MetaFunction("drop_null", cp::Arity::Unary(), stock->doc()), stock_(std::move(stock)) {}

  arrow::Result<arrow::Datum> ExecuteImpl(const std::vector<arrow::Datum>& args, const cp::FunctionOptions* options,
                                          cp::ExecContext* ctx) const override {
    if (args.size() == 1 && args[0].is_array() && DataOnRocm(*args[0].array())) {
      const ArrayData& in = *args[0].array();
      const int w = FixedByteWidth(*in.type);
      if (w == 0) return Status::NotImplemented("arrow_amd: drop_null of device-resident ", in.type->ToString(), " arrays");
      if (in.buffers[0] == nullptr || in.null_count.load() == 0 || in.length == 0) return args[0];
      hipStream_t st;
      ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
      ArxSpan dv{};
      ARROW_RETURN_NOT_OK(DeviceSpan(ArraySpan(in), &dv));
      const void* bits = dv.validity;
      dv.validity = nullptr;     // every row that survives is valid: no output bitmap
      dv.null_count = 0;
      std::shared_ptr<Buffer> values, validity;
      int64_t len = 0, nulls = 0;
      ARROW_RETURN_NOT_OK(CompactByBitmap(dv, w, bits, in.offset, in.length, st, &values, &validity, &len, &nulls));
      CountGpu(kFnFilter);
      return arrow::Datum(ArrayData::Make(in.type, len, {nullptr, std::move(values)}, 0));
    }
    return stock_->Execute(args, options, ctx);
  }

 private:
  std::shared_ptr<cp::Function> stock_;
};

// IndicesNonZero (kernels/vector_selection.cc:228-300 DoNonZero): the uint64 positions of the valid, non-zero (true)
// elements.  Device route: `values != 0` as a bitmap (arx_compare_numeric against a zero scalar; booleans are their own
// bitmap), intersected with the validity through the mask's validity (DROP), GetTakeIndices -> uint32, widened.
// Added as kernels of the live function (pyarrow's generated wrappers keep the Function object they found at import,
// so a replaced function would never be reached from pc.indices_nonzero); host arrays run the reference exec.
StockKernel g_stock_nonzero;

int NonZeroNumericTypeId(Type::type id) {
  switch (id) {
    case Type::INT8: return ARX_NUM_INT8;
    case Type::UINT8: return ARX_NUM_UINT8;
    case Type::INT16: return ARX_NUM_INT16;
    case Type::UINT16: return ARX_NUM_UINT16;
    case Type::INT32: return ARX_NUM_INT32;
    case Type::UINT32: return ARX_NUM_UINT32;
    case Type::INT64: return ARX_NUM_INT64;
    case Type::UINT64: return ARX_NUM_UINT64;
    case Type::FLOAT: return ARX_NUM_FLOAT32;
    case Type::DOUBLE: return ARX_NUM_FLOAT64;
    default: return -1;
  }
}

Status IndicesNonZeroExecRocm(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  const ArraySpan& in = batch[0].array;
  if (!OnRocm(in)) {
    CountStock(kFnFilter);
    return g_stock_nonzero.exec(ctx, batch, out);
  }
  const int64_t n = in.length;
  if (n > 0xFFFFFFFFll) return Status::NotImplemented("arrow_amd: indices_nonzero of more than UINT32_MAX device rows");
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  ArxSpan dv{};
  ARROW_RETURN_NOT_OK(DeviceSpan(in, &dv));
  ArxSpan dm{dv.validity, nullptr, dv.offset, n, dv.null_count};
  std::shared_ptr<Buffer> bits, rebased;   // (kept alive until the stream is synchronised)
  if (in.type->id() == Type::BOOL) {
    dm.data = dv.data;
  } else {
    const int num = NonZeroNumericTypeId(in.type->id());
    if (num < 0) return Status::NotImplemented("arrow_amd: indices_nonzero of device-resident ", in.type->ToString(), " arrays");
    static const int widths[10] = {1, 1, 2, 2, 4, 4, 8, 8, 4, 8};
    ARROW_ASSIGN_OR_RAISE(bits, AllocDevice(((n + 63) / 64) * 8 + 8));
    const uint64_t zero = 0;   // the all-zero bit pattern is 0 / +0.0 of every numeric type (-0.0 != 0 is false too)
    const uint8_t* base = static_cast<const uint8_t*>(dv.data) + dv.offset * widths[num];
    if (n > 0) {
      ARROW_RETURN_NOT_OK(FromArx(arx_compare_numeric(ARX_CMP_NOT_EQUAL, num, base, nullptr, nullptr, &zero, n,
                                                      reinterpret_cast<uint64_t*>(bits->mutable_address()), st)));
    }
    dm.data = reinterpret_cast<const void*>(bits->address());
    dm.offset = 0;
    if (dm.validity != nullptr && dv.offset != 0) {   // the compare output starts at bit 0: re-base the validity too
      ARROW_ASSIGN_OR_RAISE(rebased, AllocDevice(((n + 63) / 64) * 8 + 8));
      ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy(dv.validity, dv.offset, n, reinterpret_cast<void*>(rebased->mutable_address()), st)));
      dm.validity = reinterpret_cast<const void*>(rebased->address());
    }
  }
  const size_t ws_bytes = arx_filter_workspace_bytes(n);
  void* ws = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kWs, ws_bytes, &ws));
  int64_t cnt = 0;
  if (n > 0) ARROW_RETURN_NOT_OK(FromArx(arx_filter_count(&dm, ARX_FILTER_DROP, ws, ws_bytes, &cnt, st)));
  void* d_idx = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2, static_cast<size_t>(cnt) * 4 + 64, &d_idx));
  ARROW_ASSIGN_OR_RAISE(auto out_values, AllocDevice(std::max<int64_t>(cnt, 1) * 8));
  // the row numbers as uint64 straight from the gather form (round 4); the uint32 + widening pass stays as the route for
  // the forms that only write 2 / 4-byte indices (filter_sparse = 0)
  bool direct = false;
  if (cnt > 0) {
    direct = arx_mask_to_indices(&dm, ARX_FILTER_DROP, ws, cnt, 8, reinterpret_cast<void*>(out_values->mutable_address()), nullptr, st) == ARX_OK;
  }
  if (cnt > 0 && !direct) {
    ARROW_RETURN_NOT_OK(FromArx(arx_mask_to_indices(&dm, ARX_FILTER_DROP, ws, cnt, 4, d_idx, nullptr, st)));
    ArxSpan di{nullptr, d_idx, 0, cnt, 0};
    void* flag = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(kFlag, 64, &flag));
    ARROW_RETURN_NOT_OK(FromArx(arx_cast_numeric(&di, ARX_NUM_UINT32, ARX_NUM_UINT64, 1, 1, flag, 64,
                                                 reinterpret_cast<void*>(out_values->mutable_address()), st)));
  }
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  CountGpu(kFnFilter);
  out->value = ArrayData::Make(arrow::uint64(), cnt, {nullptr, std::move(out_values)}, 0);
  return Status::OK();
}

Status RegisterIndicesNonZero(cp::FunctionRegistry* reg) {
  ARROW_ASSIGN_OR_RAISE(auto fn, reg->GetFunction("indices_nonzero"));
  if (fn->kind() != cp::Function::VECTOR) return Status::Invalid("indices_nonzero is not a vector function");
  auto* vfn = static_cast<cp::VectorFunction*>(fn.get());
  for (const auto& ty : {arrow::boolean(), arrow::int8(), arrow::uint8(), arrow::int16(), arrow::uint16(), arrow::int32(),
                         arrow::uint32(), arrow::int64(), arrow::uint64(), arrow::float32(), arrow::float64()}) {
    ARROW_ASSIGN_OR_RAISE(const cp::Kernel* k0, vfn->DispatchExact({ty}));
    cp::VectorKernel copy = *static_cast<const cp::VectorKernel*>(k0);
    if (g_stock_nonzero.exec == nullptr) g_stock_nonzero.exec = copy.exec;
    if (g_stock_nonzero.exec != copy.exec) continue;
    copy.exec = IndicesNonZeroExecRocm;   // (exec_chunked stays the reference's: chunked host arrays)
    ARROW_RETURN_NOT_OK(vfn->AddKernel(std::move(copy)));
  }
  return Status::OK();
}

// fixed-width types the Grouper takes as one key column (bits compared, like the reference's physical-type memo tables)
struct HashValueType {
  std::shared_ptr<arrow::DataType> probe;
  cp::InputType match;
};
std::vector<HashValueType> HashVectorTypes() {
  using arrow::TimeUnit;
  std::vector<HashValueType> t;
  for (const auto& ty : {arrow::int8(), arrow::uint8(), arrow::int16(), arrow::uint16(), arrow::int32(), arrow::uint32(),
                         arrow::int64(), arrow::uint64(), arrow::float32(), arrow::float64(), arrow::date32(), arrow::date64()}) {
    t.push_back({ty, cp::InputType(ty)});
  }
  t.push_back({arrow::time32(TimeUnit::SECOND), cp::InputType(Type::TIME32)});
  t.push_back({arrow::time64(TimeUnit::NANO), cp::InputType(Type::TIME64)});
  t.push_back({arrow::timestamp(TimeUnit::NANO), cp::InputType(Type::TIMESTAMP)});
  t.push_back({arrow::duration(TimeUnit::NANO), cp::InputType(Type::DURATION)});
  return t;
}

template <HashVectorKind KIND>
Status RegisterHashVector(cp::FunctionRegistry* reg, const char* name, StockKernel* stock,
                          cp::VectorKernel::FinalizeFunc* stock_finalize) {
  ARROW_ASSIGN_OR_RAISE(auto fn, reg->GetFunction(name));
  if (fn->kind() != cp::Function::VECTOR) return Status::Invalid(name, " is not a vector function");
  auto* vfn = static_cast<cp::VectorFunction*>(fn.get());
  const std::vector<HashValueType> types = HashVectorTypes();
  for (const auto& vt : types) {
    ARROW_ASSIGN_OR_RAISE(const cp::Kernel* k0, vfn->DispatchExact({vt.probe}));
    cp::VectorKernel copy = *static_cast<const cp::VectorKernel*>(k0);
    if (stock->exec == nullptr) {
      stock->exec = copy.exec;
      *stock_finalize = copy.finalize;
    } else if (stock->exec != copy.exec) {
      continue;   // a different stock kernel handles this type: leave it alone
    }
    // every type has its own stock init (GetHashInit picks the memo table): keep it per added kernel
    stock->init = nullptr;
    const cp::KernelInit stock_init = copy.init;
    copy.init = [stock_init](cp::KernelContext* ctx, const cp::KernelInitArgs& args)
        -> arrow::Result<std::unique_ptr<cp::KernelState>> {
      auto state = std::make_unique<DeviceHashState>();
      state->kind = KIND;
      state->type = args.inputs[0].GetSharedPtr();
      state->width = FixedByteWidth(*state->type);
      if (KIND == kHashDictEncode && args.options != nullptr) {
        state->encode_nulls = static_cast<const cp::DictionaryEncodeOptions*>(args.options)->null_encoding_behavior ==
                              cp::DictionaryEncodeOptions::ENCODE;
      }
      ARROW_ASSIGN_OR_RAISE(state->stock, stock_init(ctx, args));
      return state;
    };
    copy.signature = cp::KernelSignature::Make({vt.match}, copy.signature->out_type());
    copy.exec = HashVectorExec<KIND>;
    copy.finalize = HashVectorFinalize<KIND>;
    copy.mem_allocation = cp::MemAllocation::NO_PREALLOCATE;
    ARROW_RETURN_NOT_OK(vfn->AddKernel(std::move(copy)));
  }
  return Status::OK();
}

// array_sort_indices shims.
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- array_sort_indices(uint64|int64)
// One slot per registered value type: 0-5 = the ARX_KEY_* types themselves, 6-11 = temporal types
// sorted by their physical integer (date32, date64, timestamp, duration, time32, time64), 12-15 = int8 / uint8 /
// int16 / uint16: device-resident arrays are sign- / zero-extended to 32 bits on the device and sorted as such (the
// reference counts these on the CPU, vector_array_sort.cc ArrayCountSorter — host arrays keep that kernel).
// 16 = decimal128: device-resident arrays are sorted as the key pair (high word int64, low word uint64) by the chain of
// plugin/order_by_node.inc (DecimalSortOnDevice); host arrays keep the reference's kernel.
// 17 / 18 = utf8 / binary: likewise as (8-byte big-endian chunks, length) keys (SplitBinaryKeyOnDevice).
// 19 = boolean (round 6): device-resident arrays are sorted by COUNTING, as the reference does on the CPU
// (ArrayCountSorter<BooleanType>, vector_array_sort.cc:360-400): the rows of the falses, of the trues and of the nulls, each in
// row order (three GetTakeIndices over the value bitmap, its inverse and the inverted validity), laid one behind the other.
// 20 = dictionary (round 6): the reference's own algorithm (ArrayCompareSorter<DictionaryType>, vector_array_sort.cc:180-265)
// with the big steps on the device — dense ranks of the dictionary VALUES (small: ranked by the stock "rank" on a host copy,
// any value type the reference ranks), ranks uploaded, Take(ranks, indices) and the sort of the decoded uint64 ranks in HBM.
// 21 / 22 = large_utf8 / large_binary (round 6): int64 offsets narrowed to int32 on the device (columns of less than 2 GB of
// bytes), then the utf8 / binary chain.
// 23 = struct (round 6): the null structs to their end, the others by the multi-key chain over the fields (the reference:
// ArrayCompareSorter<StructType> -> SortStructArray).
constexpr int kSortSlots = 24;
constexpr int kSortSlotStruct = 23;
constexpr int kSortSlotDecimal = 16;
constexpr int kSortSlotUtf8 = 17;
constexpr int kSortSlotBinary = 18;
constexpr int kSortSlotBoolean = 19;
constexpr int kSortSlotDictionary = 20;
constexpr int kSortSlotLargeUtf8 = 21;
constexpr int kSortSlotLargeBinary = 22;
constexpr int kSortSlotKey[kSortSlots] = {ARX_KEY_UINT64, ARX_KEY_INT64, ARX_KEY_UINT32, ARX_KEY_INT32,
                                          ARX_KEY_FLOAT64, ARX_KEY_FLOAT32, ARX_KEY_INT32, ARX_KEY_INT64,
                                          ARX_KEY_INT64, ARX_KEY_INT64, ARX_KEY_INT32, ARX_KEY_INT64,
                                          ARX_KEY_INT32, ARX_KEY_UINT32, ARX_KEY_INT32, ARX_KEY_UINT32, ARX_KEY_INT64,
                                          ARX_KEY_UINT64, ARX_KEY_UINT64, ARX_KEY_UINT32, ARX_KEY_UINT64, ARX_KEY_UINT64, ARX_KEY_UINT64,
                                          ARX_KEY_UINT64};
// the element type a slot's values are widened FROM (-1: sorted as they are; -2: decimal128 / utf8 / binary — the key chain;
// -3: boolean — the counting sort; -4: dictionary — ranks of the values, then the ranks' sort; -5: struct — its fields as keys)
constexpr int kSortSlotNarrow[kSortSlots] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
                                             ARX_NUM_INT8, ARX_NUM_UINT8, ARX_NUM_INT16, ARX_NUM_UINT16, -2, -2, -2, -3, -4, -2, -2, -5};
Status DecimalSortOnDevice(const ArraySpan& values, const cp::ArraySortOptions& options, cp::ExecContext* ctx, ArrayData* out);
Status BooleanSortOnDevice(const ArraySpan& values, const cp::ArraySortOptions& options, cp::ExecContext* ctx, ArrayData* out);
Status DictionarySortOnDevice(const ArraySpan& values, const cp::ArraySortOptions& options, cp::ExecContext* ctx, ArrayData* out);
Status StructSortOnDevice(const ArraySpan& values, const cp::ArraySortOptions& options, cp::ExecContext* ctx, ArrayData* out);
StockKernel g_stock_sort[kSortSlots];

arrow::Result<std::unique_ptr<cp::KernelState>> SortInitImpl(const StockKernel& stock,
                                                             cp::KernelContext* ctx,
                                                             const cp::KernelInitArgs& args) {
  auto state = std::make_unique<ShimState<cp::ArraySortOptions>>();
  if (stock.init) {
    ARROW_ASSIGN_OR_RAISE(state->stock, stock.init(ctx, args));
  }
  if (args.options != nullptr) state->options = *static_cast<const cp::ArraySortOptions*>(args.options);
  return state;
}
template <int K>
arrow::Result<std::unique_ptr<cp::KernelState>> SortInitT(cp::KernelContext* c, const cp::KernelInitArgs& a) {
  return SortInitImpl(g_stock_sort[K], c, a);
}

// ArraySortIndices::Exec (vector_array_sort.cc:524-540): output uint64 is preallocated.
Status SortExecImpl(const StockKernel& stock, int key_type, int narrow_from, cp::KernelContext* ctx,
                    const cp::ExecSpan& batch, cp::ExecResult* out) {
  auto* state = static_cast<ShimState<cp::ArraySortOptions>*>(ctx->state());
  const ArraySpan& values = batch[0].array;
  if (values.length < g_min_rows.load() || !IsHost(values) || narrow_from >= 0 || narrow_from <= -2) {   // (host int8 / int16 / booleans: the counting sort; host decimals)
    return RunStock(kFnSort, stock, state->stock.get(), ctx, batch, out);
  }
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  ArxSpan dv{};
  const int key_width = (key_type == ARX_KEY_UINT32 || key_type == ARX_KEY_INT32 || key_type == ARX_KEY_FLOAT32) ? 4 : 8;
  ARROW_RETURN_NOT_OK(Upload(values, key_width, kValues, kValidity, st, &dv));
  const int64_t n = values.length;
  const size_t ws_bytes = arx_sort_indices_workspace_bytes(n);
  void *ws = nullptr, *dout = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kWs, ws_bytes, &ws));
  ARROW_RETURN_NOT_OK(t_scratch.Get(kOutData, static_cast<size_t>(n) * 8, &dout));
  const int order = state->options.order == cp::SortOrder::Descending ? ARX_SORT_DESCENDING : ARX_SORT_ASCENDING;
  const int placement = state->options.null_placement == cp::NullPlacement::AtStart ? ARX_NULLS_AT_START
                                                                                    : ARX_NULLS_AT_END;
  ARROW_RETURN_NOT_OK(FromArx(arx_sort_indices(&dv, key_type, order, placement, ws, ws_bytes,
                                                  static_cast<uint64_t*>(dout), st)));
  uint64_t* host_out = nullptr;
  if (out->is_array_span()) {
    host_out = out->array_span_mutable()->GetValues<uint64_t>(1);
  } else {
    host_out = out->array_data()->GetMutableValues<uint64_t>(1);
  }
  HIP_RETURN_NOT_OK(hipMemcpyAsync(host_out, dout, static_cast<size_t>(n) * 8, hipMemcpyDeviceToHost, st));
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  CountGpu(kFnSort);
  return Status::OK();
}
// The registered kernels are MemAllocation::NO_PREALLOCATE twins (the stock ones preallocate the
// uint64 output from the CPU pool, vector_array_sort.cc:656-657): device-resident input sorts in
// HBM and the indices stay there; host input gets the buffer the executor would have preallocated
// and runs the preallocated-style exec above.
Status SortExecNP(const StockKernel& stock, int key_type, int narrow_from, cp::KernelContext* ctx, const cp::ExecSpan& batch,
                  cp::ExecResult* out) {
  const ArraySpan& values = batch[0].array;
  const int64_t n = values.length;
  ArrayData* out_arr = out->array_data().get();
  out_arr->buffers.resize(2);
  out_arr->buffers[0] = nullptr;
  out_arr->length = n;
  out_arr->null_count = 0;
  if (narrow_from == -5 && SpanTouchesRocm(values)) {
    auto* state = static_cast<ShimState<cp::ArraySortOptions>*>(ctx->state());
    ARROW_RETURN_NOT_OK(StructSortOnDevice(values, state->options, ctx->exec_context(), out_arr));
    CountGpu(kFnSort);
    return Status::OK();
  }
  if (narrow_from == -4 && OnRocm(values)) {
    auto* state = static_cast<ShimState<cp::ArraySortOptions>*>(ctx->state());
    ARROW_RETURN_NOT_OK(DictionarySortOnDevice(values, state->options, ctx->exec_context(), out_arr));
    CountGpu(kFnSort);
    return Status::OK();
  }
  if (narrow_from == -3 && OnRocm(values)) {
    auto* state = static_cast<ShimState<cp::ArraySortOptions>*>(ctx->state());
    ARROW_RETURN_NOT_OK(BooleanSortOnDevice(values, state->options, ctx->exec_context(), out_arr));
    CountGpu(kFnSort);
    return Status::OK();
  }
  if (narrow_from == -2 && (OnRocm(values) || (values.type->id() != Type::DECIMAL128 && OnRocm3(values)))) {
    auto* state = static_cast<ShimState<cp::ArraySortOptions>*>(ctx->state());
    ARROW_RETURN_NOT_OK(DecimalSortOnDevice(values, state->options, ctx->exec_context(), out_arr));
    CountGpu(kFnSort);
    return Status::OK();
  }
  if (OnRocm(values)) {
    auto* state = static_cast<ShimState<cp::ArraySortOptions>*>(ctx->state());
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    ArxSpan dv{};
    ARROW_RETURN_NOT_OK(DeviceSpan(values, &dv));
    if (narrow_from >= 0 && n > 0) {
      // int8 ... uint16 keys: widened to int32 / uint32 (order-preserving), the validity bits moved to bit 0 beside them
      void *wide = nullptr, *flag = nullptr, *bits = nullptr;
      ARROW_RETURN_NOT_OK(t_scratch.Get(kValues, static_cast<size_t>(n) * 4 + 16, &wide));
      ARROW_RETURN_NOT_OK(t_scratch.Get(kFlag, 64, &flag));
      ARROW_RETURN_NOT_OK(FromArx(arx_cast_numeric(&dv, narrow_from, key_type == ARX_KEY_UINT32 ? ARX_NUM_UINT32 : ARX_NUM_INT32,
                                                   /*allow_int_overflow=*/1, /*allow_float_truncate=*/1, flag, 8, wide, st)));
      if (dv.validity != nullptr) {
        ARROW_RETURN_NOT_OK(t_scratch.Get(kValidity, static_cast<size_t>((n + 63) / 64) * 8 + 16, &bits));
        ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy(dv.validity, dv.offset, n, bits, st)));
      }
      dv.data = wide;
      dv.validity = bits;
      dv.offset = 0;
    }
    const size_t ws_bytes = arx_sort_indices_workspace_bytes(n);
    void* ws = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(kWs, ws_bytes, &ws));
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice(n * 8));
    const int order = state->options.order == cp::SortOrder::Descending ? ARX_SORT_DESCENDING : ARX_SORT_ASCENDING;
    const int placement = state->options.null_placement == cp::NullPlacement::AtStart ? ARX_NULLS_AT_START
                                                                                      : ARX_NULLS_AT_END;
    ARROW_RETURN_NOT_OK(FromArx(arx_sort_indices(&dv, key_type, order, placement, ws, ws_bytes,
                                                    reinterpret_cast<uint64_t*>(out_arr->buffers[1]->mutable_address()),
                                                    st)));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    CountGpu(kFnSort);
    return Status::OK();
  }
  ARROW_ASSIGN_OR_RAISE(std::shared_ptr<Buffer> data, ctx->Allocate(n * 8));
  // the VectorExecutor hands vector kernels an ArrayData (exec.cc:1103-1111): same shape here
  cp::ExecResult tmp;
  tmp.value = ArrayData::Make(out_arr->type, n, {nullptr, data}, /*null_count=*/0);
  ARROW_RETURN_NOT_OK(SortExecImpl(stock, key_type, narrow_from, ctx, batch, &tmp));
  out_arr->buffers[1] = std::move(data);
  return Status::OK();
}
// Chunked input goes to the stock exec_chunked (ArraySortIndicesChunked), which expects the
// preallocated output our NO_PREALLOCATE twin no longer gets from the executor: allocate it here.
Status SortChunkedNP(const StockKernel& stock, cp::KernelContext* ctx, const cp::ExecBatch& batch, arrow::Datum* out) {
  auto* state = static_cast<ShimState<cp::ArraySortOptions>*>(ctx->state());
  ArrayData* out_arr = out->mutable_array();
  out_arr->buffers.resize(2);
  out_arr->buffers[0] = nullptr;
  ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], ctx->Allocate(batch.length * 8));
  out_arr->null_count = 0;
  return RunStock(kFnSort, stock.exec_chunked, std::optional<cp::KernelState*>(state->stock.get()), ctx, batch, out);
}
template <int K>
Status SortChunkedT(cp::KernelContext* c, const cp::ExecBatch& b, arrow::Datum* o) {
  return SortChunkedNP(g_stock_sort[K], c, b, o);
}
template <int K>
Status SortExecT(cp::KernelContext* c, const cp::ExecSpan& b, cp::ExecResult* o) {
  return SortExecNP(g_stock_sort[K], kSortSlotKey[K], kSortSlotNarrow[K], c, b, o);
}

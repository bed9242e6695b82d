// array_filter / array_take shims: fixed-width (host staging + device) and utf8/binary (device).
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- filter
StockKernel g_stock_filter;

arrow::Result<std::unique_ptr<cp::KernelState>> FilterInit(cp::KernelContext* ctx,
                                                           const cp::KernelInitArgs& args) {
  auto state = std::make_unique<ShimState<cp::FilterOptions>>();
  if (g_stock_filter.init) {
    ARROW_ASSIGN_OR_RAISE(state->stock, g_stock_filter.init(ctx, args));
  }
  if (args.options != nullptr) {
    state->options = *static_cast<const cp::FilterOptions*>(args.options);
  }
  return state;
}

// take on BOOLEAN (bit-packed) values that live on the device: value bits and validity come out of
// arx_take_bits as two bitmaps; a filter is arx_mask_to_indices + this (like the var-width types)
Status BooleanTakeOnDevice(const ArxSpan& dv, const ArxSpan& di, int tid, hipStream_t st, ArrayData* out_arr) {
  const int64_t m = di.length;
  const int64_t bytes = ((m + 63) / 64) * 8;
  const bool allocate_validity = dv.null_count != 0 || di.null_count != 0;
  out_arr->length = m;
  out_arr->buffers.resize(2);
  out_arr->buffers[0] = nullptr;
  ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice(bytes));
  void* d_valid = nullptr;
  void* d_counter = nullptr;
  if (allocate_validity) {
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[0], AllocDevice(bytes));
    d_valid = reinterpret_cast<void*>(out_arr->buffers[0]->mutable_address());
    ARROW_RETURN_NOT_OK(t_scratch.Get(kCounter, 64, &d_counter));
    HIP_RETURN_NOT_OK(hipMemsetAsync(d_counter, 0, 8, st));
  }
  ARROW_RETURN_NOT_OK(FromArx(arx_take_bits(&dv, &di, tid, reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address()),
                                            d_valid, static_cast<int64_t*>(d_counter), st)));
  int64_t valid_count = m;
  if (allocate_validity) HIP_RETURN_NOT_OK(hipMemcpyAsync(&valid_count, d_counter, 8, hipMemcpyDeviceToHost, st));
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  out_arr->null_count = m - valid_count;
  return Status::OK();
}

// A run_end_encoded<int16/32/64, boolean> filter in HBM -> the plain mask layout the filter kernels take
// (arx_ree_bool_expand: every row of a run carries its run's (valid, selected) pair, exactly what the reference's run
// visitor walks, vector_selection_internal.cc:79-153), in this thread's scratch.  PrimitiveFilterExec takes REE filters
// through the same exec (vector_selection_filter_internal.cc:448,1090,1116).
bool ReeFilterOnRocm(const ArraySpan& filter) {
  return filter.type->id() == Type::RUN_END_ENCODED && filter.child_data.size() == 2 &&
         OnRocm(filter.child_data[0]) && OnRocm(filter.child_data[1]);
}
Status ExpandReeFilterOnDevice(const ArraySpan& filter, hipStream_t st, ArxSpan* dm) {
  const ArraySpan& run_ends = filter.child_data[0];
  const ArraySpan& run_values = filter.child_data[1];
  const int rw = FixedByteWidth(*run_ends.type);
  if (run_values.type->id() != Type::BOOL || (rw != 2 && rw != 4 && rw != 8)) {
    return Status::NotImplemented("arrow_amd: filter of type ", filter.type->ToString());
  }
  ArxSpan ends{}, vals{};
  ARROW_RETURN_NOT_OK(DeviceSpan(run_ends, &ends));
  ARROW_RETURN_NOT_OK(DeviceSpan(run_values, &vals));
  const int64_t n = filter.length;
  const size_t bytes = static_cast<size_t>((n + 63) / 64) * 8 + 64;
  void *d_bits = nullptr, *d_valid = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2, bytes, &d_bits));
  const bool may_have_nulls = vals.validity != nullptr && vals.null_count != 0;
  if (may_have_nulls) ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2Validity, bytes, &d_valid));
  ARROW_RETURN_NOT_OK(FromArx(arx_ree_bool_expand(static_cast<const uint8_t*>(ends.data) + ends.offset * rw, rw, run_ends.length,
                                                  &vals, filter.offset, n, d_bits, d_valid, st)));
  *dm = ArxSpan{d_valid, d_bits, 0, n, may_have_nulls ? arrow::kUnknownNullCount : 0};
  return Status::OK();
}

// PrimitiveFilterExec (vector_selection_filter_internal.cc:445-510) with the loop on the GPU.
Status FilterExec(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  auto* state = static_cast<ShimState<cp::FilterOptions>*>(ctx->state());
  const ArraySpan& values = batch[0].array;
  const ArraySpan& filter = batch[1].array;
  const int w = FixedByteWidth(*values.type);
  const int null_sel = state->options.null_selection_behavior == cp::FilterOptions::EMIT_NULL
                           ? ARX_FILTER_EMIT_NULL : ARX_FILTER_DROP;
  const bool ree = filter.type->id() == Type::RUN_END_ENCODED;
  const bool on_device = OnRocm(values) || OnRocm(filter) || (ree && ReeFilterOnRocm(filter));
  if (on_device && ree && (!OnRocm(values) || !ReeFilterOnRocm(filter))) {
    return Status::NotImplemented("arrow_amd: a run-end encoded filter and its values must both be device-resident");
  }
  if (on_device) {
    // device-resident ExecBatch: no staging, the output stays in HBM
    if (values.type->id() == Type::BOOL && ree) {
      return Status::NotImplemented("arrow_amd: run-end encoded filter of boolean values on device-resident arrays");
    }
    if (values.type->id() == Type::BOOL && filter.type->id() == Type::BOOL) {
      if (filter.length > 0xFFFFFFFFll) {
        return Status::NotImplemented("Filter length exceeds UINT32_MAX, consider a different strategy for selecting elements");
      }
      hipStream_t st;
      ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
      ArxSpan dv{}, dm{};
      ARROW_RETURN_NOT_OK(DeviceSpan(values, &dv));
      ARROW_RETURN_NOT_OK(DeviceSpan(filter, &dm));
      const size_t ws_bytes = arx_filter_workspace_bytes(filter.length);
      void* ws = nullptr;
      ARROW_RETURN_NOT_OK(t_scratch.Get(kWs, ws_bytes, &ws));
      int64_t out_len = 0;
      ARROW_RETURN_NOT_OK(FromArx(arx_filter_count(&dm, null_sel, ws, ws_bytes, &out_len, st)));
      const bool emit = null_sel == ARX_FILTER_EMIT_NULL && dm.null_count != 0;
      void* d_idx = nullptr;
      void* d_idx_valid = nullptr;
      ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2, static_cast<size_t>(out_len) * 4 + 64, &d_idx));
      if (emit) ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2Validity, static_cast<size_t>((out_len + 63) / 64) * 8 + 64, &d_idx_valid));
      ARROW_RETURN_NOT_OK(FromArx(arx_mask_to_indices(&dm, null_sel, ws, out_len, 4, d_idx, d_idx_valid, st)));
      ArxSpan di{d_idx_valid, d_idx, 0, out_len, emit ? arrow::kUnknownNullCount : 0};
      ARROW_RETURN_NOT_OK(BooleanTakeOnDevice(dv, di, ARX_UINT32, st, out->array_data().get()));
      CountGpu(kFnFilter);
      return Status::OK();
    }
    if (w == 0 || (filter.type->id() != Type::BOOL && !ree)) {
      return Status::NotImplemented("arrow_amd: filter of ", values.type->ToString(),
                                    " on device-resident arrays");
    }
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    ArxSpan dv{}, dm{};
    ARROW_RETURN_NOT_OK(DeviceSpan(values, &dv));
    if (ree) {
      ARROW_RETURN_NOT_OK(ExpandReeFilterOnDevice(filter, st, &dm));
    } else {
      ARROW_RETURN_NOT_OK(DeviceSpan(filter, &dm));
    }
    const size_t ws_bytes = arx_filter_workspace_bytes(filter.length);
    void* ws = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(kWs, ws_bytes, &ws));
    ArrayData* out_arr = out->array_data().get();
    const bool allocate_validity = dv.null_count != 0 || dm.null_count != 0;
    if (filter.length > 0 && filter.length <= g_filter_morsel_rows.load()) {
      // Morsel-sized input (Acero hands over <= 32Ki rows per batch): the host round trips cost more than the
      // kernels.  Allocate for the worst case (every row selected), run count -> compact back to back, and read
      // the output length and the null count back with ONE synchronisation instead of three.
      const int64_t n = filter.length;
      ARROW_RETURN_NOT_OK(FromArx(arx_filter_count_async(&dm, null_sel, ws, ws_bytes, st)));
      out_arr->buffers.resize(2);
      ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice(n * w));
      out_arr->buffers[0] = nullptr;
      void* d_valid = nullptr;
      if (allocate_validity) {
        ARROW_ASSIGN_OR_RAISE(out_arr->buffers[0], AllocDevice(((n + 63) / 64) * 8));
        d_valid = reinterpret_cast<void*>(out_arr->buffers[0]->mutable_address());
      }
      // (out_length = n: all ceil(n/64) validity words are cleared first, so bits past the real length stay zero)
      ARROW_RETURN_NOT_OK(FromArx(arx_filter_exec(&dv, w, &dm, null_sel, ws, n,
                                                  reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address()),
                                                  d_valid, st)));
      int64_t selected = 0, set_bits = 0;
      HIP_RETURN_NOT_OK(hipMemcpyAsync(&selected, ws, 8, hipMemcpyDeviceToHost, st));   // arx_filter_count_async left it there
      if (allocate_validity) {
        void* cws = nullptr;
        ARROW_RETURN_NOT_OK(t_scratch.Get(kCounter, 64, &cws));
        ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_popcount(d_valid, 0, n, cws, 64, &set_bits, st)));   // synchronises
      } else {
        HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
      }
      out_arr->length = selected;
      out_arr->null_count = allocate_validity ? selected - set_bits : 0;
      static_cast<RocmBuffer*>(out_arr->buffers[1].get())->Shrink(selected * w);
      if (allocate_validity) static_cast<RocmBuffer*>(out_arr->buffers[0].get())->Shrink(((selected + 63) / 64) * 8);
      CountGpu(kFnFilter);
      return Status::OK();
    }
    // the output's length AND its null count from the one counting pass and its one read-back (the popcount kernel + a
    // second read-back after the compaction were ~70 us of the 1.5 ms headline filter: profiles/r04_o_*)
    int64_t out_len = 0, out_nulls = 0;
    if (allocate_validity) {
      ARROW_RETURN_NOT_OK(FromArx(arx_filter_count_nulls(&dv, &dm, null_sel, ws, ws_bytes, &out_len, &out_nulls, st)));
    } else {
      ARROW_RETURN_NOT_OK(FromArx(arx_filter_count(&dm, null_sel, ws, ws_bytes, &out_len, st)));
    }
    out_arr->length = out_len;
    out_arr->buffers.resize(2);
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice(out_len * w));
    out_arr->buffers[0] = nullptr;
    void* d_valid = nullptr;
    if (allocate_validity) {
      ARROW_ASSIGN_OR_RAISE(out_arr->buffers[0], AllocDevice(((out_len + 63) / 64) * 8));
      d_valid = reinterpret_cast<void*>(out_arr->buffers[0]->mutable_address());
    }
    ARROW_RETURN_NOT_OK(FromArx(arx_filter_exec(&dv, w, &dm, null_sel, ws, out_len,
                                                reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address()),
                                                d_valid, st)));
    out_arr->null_count = allocate_validity ? out_nulls : 0;
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    CountGpu(kFnFilter);
    return Status::OK();
  }
  if (w == 0 || filter.type->id() != Type::BOOL || values.length < g_min_rows.load() ||
      !IsHost(values) || !IsHost(filter)) {
    return RunStock(kFnFilter, g_stock_filter, state->stock.get(), ctx, batch, out);
  }
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  ArxSpan dv{}, dm{};
  ARROW_RETURN_NOT_OK(Upload(values, w, kValues, kValidity, st, &dv));
  ARROW_RETURN_NOT_OK(Upload(filter, 0, kArg2, kArg2Validity, st, &dm));
  const size_t ws_bytes = arx_filter_workspace_bytes(filter.length);
  void* ws = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kWs, ws_bytes, &ws));
  int64_t out_len = 0;
  ARROW_RETURN_NOT_OK(FromArx(arx_filter_count(&dm, null_sel, ws, ws_bytes, &out_len, st)));

  ArrayData* out_arr = out->array_data().get();
  const bool filter_null_count_is_zero = filter.null_count == 0;
  if (values.null_count == 0 && (null_sel == ARX_FILTER_DROP || filter_null_count_is_zero)) {
    out_arr->null_count = 0;
  } else {
    out_arr->null_count = arrow::kUnknownNullCount;
  }
  const bool allocate_validity = values.null_count != 0 || !filter_null_count_is_zero;
  out_arr->length = out_len;
  out_arr->buffers.resize(2);
  ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], ctx->Allocate(out_len * w));
  void* d_out = nullptr;
  void* d_out_valid = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kOutData, static_cast<size_t>(out_len) * w + 16, &d_out));
  const size_t vbytes = static_cast<size_t>((out_len + 63) / 64) * 8;
  if (allocate_validity) {
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[0], ctx->AllocateBitmap(out_len));
    ARROW_RETURN_NOT_OK(t_scratch.Get(kOutValidity, vbytes + 16, &d_out_valid));
  } else {
    out_arr->buffers[0] = nullptr;
  }
  ARROW_RETURN_NOT_OK(FromArx(arx_filter_exec(&dv, w, &dm, null_sel, ws, out_len, d_out, d_out_valid, st)));
  if (out_len > 0) {
    HIP_RETURN_NOT_OK(hipMemcpyAsync(out_arr->buffers[1]->mutable_data(), d_out,
                                     static_cast<size_t>(out_len) * w, hipMemcpyDeviceToHost, st));
    if (allocate_validity) {
      HIP_RETURN_NOT_OK(hipMemcpyAsync(out_arr->buffers[0]->mutable_data(), d_out_valid,
                                       static_cast<size_t>(arrow::bit_util::BytesForBits(out_len)),
                                       hipMemcpyDeviceToHost, st));
    }
  }
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  CountGpu(kFnFilter);
  return Status::OK();
}

int IndexTypeId(const arrow::DataType& t);

// ---------------------------------------------------------------- binary / utf8 (device-resident)
// TakeExec / FilterExec for base binary on arrays that live in HBM: the offsets/validity pass,
// one 8-byte read-back of the byte total (the reference grows a builder instead), then the bytes.
// Host-resident strings stay on the stock kernels (they would be PCIe-bound both ways).
StockKernel g_stock_filter_bin, g_stock_take_bin, g_stock_filter_large_bin, g_stock_take_large_bin;   // (large_: int64 offsets)

arrow::Result<std::unique_ptr<cp::KernelState>> BinaryFilterInit(cp::KernelContext* ctx,
                                                                 const cp::KernelInitArgs& args) {
  auto state = std::make_unique<ShimState<cp::FilterOptions>>();
  const bool large_in = !args.inputs.empty() && args.inputs[0].type != nullptr && BinaryOffsetWidth(args.inputs[0].type->id()) == 8;
  const StockKernel& stock_k = large_in ? g_stock_filter_large_bin : g_stock_filter_bin;
  if (stock_k.init) {
    ARROW_ASSIGN_OR_RAISE(state->stock, stock_k.init(ctx, args));
  }
  if (args.options != nullptr) state->options = *static_cast<const cp::FilterOptions*>(args.options);
  return state;
}

arrow::Result<std::unique_ptr<cp::KernelState>> BinaryTakeInit(cp::KernelContext* ctx,
                                                               const cp::KernelInitArgs& args) {
  auto state = std::make_unique<ShimState<cp::TakeOptions>>();
  const bool large_in = !args.inputs.empty() && args.inputs[0].type != nullptr && BinaryOffsetWidth(args.inputs[0].type->id()) == 8;
  const StockKernel& stock_k = large_in ? g_stock_take_large_bin : g_stock_take_bin;
  if (stock_k.init) {
    ARROW_ASSIGN_OR_RAISE(state->stock, stock_k.init(ctx, args));
  }
  if (args.options != nullptr) state->options = *static_cast<const cp::TakeOptions*>(args.options);
  return state;
}

// CheckIndexBounds (util/int_util.cc:530-587) on device-resident indices: IndexError naming the first offender
Status CheckBoundsOnDevice(const ArxSpan& indices, int index_type, int64_t values_length, hipStream_t st) {
  void* ws = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kWs, arx_take_workspace_bytes(), &ws));
  return FromArx(arx_check_index_bounds(&indices, index_type, static_cast<uint64_t>(values_length), ws,
                                        arx_take_workspace_bytes(), st));
}

bool OnRocm3(const ArraySpan& a) {
  if (OnRocm(a)) return true;
  return a.buffers[2].owner != nullptr && *a.buffers[2].owner != nullptr &&
         (*a.buffers[2].owner)->device_type() == arrow::DeviceAllocationType::kROCM;
}

Status DeviceBinarySpan(const ArraySpan& a, ArxBinarySpan* out) {
  const void* addr[3] = {nullptr, nullptr, nullptr};
  for (int i = 0; i < 3; ++i) {
    const auto* owner = a.buffers[i].owner;
    if (owner == nullptr || *owner == nullptr) continue;
    if ((*owner)->device_type() != arrow::DeviceAllocationType::kROCM) {
      return Status::Invalid("arrow_amd: mixed host / device buffers in one array");
    }
    addr[i] = reinterpret_cast<const void*>((*owner)->address());
  }
  out->validity = addr[0];
  out->offsets = static_cast<const int32_t*>(addr[1]);
  out->data = addr[2];
  out->offset = a.offset;
  out->length = a.length;
  out->null_count = addr[0] == nullptr ? 0 : (a.null_count > 0 ? a.null_count : arrow::kUnknownNullCount);
  return Status::OK();
}

// large: int64 offsets (large_utf8 / large_binary; dv.offsets then points at int64 entries)
Status BinaryTakeOnDevice(const ArxBinarySpan& dv, const ArxSpan& di, int tid, hipStream_t st, ArrayData* out_arr, bool large = false) {
  const int64_t m = di.length;
  const bool allocate_validity = dv.null_count != 0 || di.null_count != 0;
  out_arr->length = m;
  out_arr->buffers.resize(3);
  out_arr->buffers[0] = nullptr;
  ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice((m + 1) * (large ? 8 : 4)));
  void* d_valid = nullptr;
  void* d_counter = nullptr;
  if (allocate_validity) {
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[0], AllocDevice(((m + 63) / 64) * 8));
    d_valid = reinterpret_cast<void*>(out_arr->buffers[0]->mutable_address());
    ARROW_RETURN_NOT_OK(t_scratch.Get(kCounter, 64, &d_counter));
    HIP_RETURN_NOT_OK(hipMemsetAsync(d_counter, 0, 8, st));
  }
  const size_t ws_bytes = large ? arx_large_binary_take_workspace_bytes(m) : arx_binary_take_workspace_bytes(m);
  void* ws = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kBinWs, ws_bytes, &ws));
  void* d_off = reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address());
  int64_t total = 0;
  if (large) {
    ARROW_RETURN_NOT_OK(FromArx(arx_large_binary_take_offsets(&dv, &di, tid, ws, ws_bytes, static_cast<int64_t*>(d_off), d_valid,
                                                              static_cast<int64_t*>(d_counter), &total, st)));
  } else {
    ARROW_RETURN_NOT_OK(FromArx(arx_binary_take_offsets(&dv, &di, tid, ws, ws_bytes, static_cast<int32_t*>(d_off), d_valid,
                                                        static_cast<int64_t*>(d_counter), &total, st)));
  }
  ARROW_ASSIGN_OR_RAISE(out_arr->buffers[2], AllocDevice(total));
  void* d_data = reinterpret_cast<void*>(out_arr->buffers[2]->mutable_address());
  if (large) {
    ARROW_RETURN_NOT_OK(FromArx(arx_large_binary_take_data(&dv, m, ws, ws_bytes, static_cast<const int64_t*>(d_off), total, d_data, st)));
  } else {
    ARROW_RETURN_NOT_OK(FromArx(arx_binary_take_data(&dv, m, ws, ws_bytes, static_cast<const int32_t*>(d_off), total, d_data, st)));
  }
  int64_t valid_count = m;
  if (allocate_validity) {
    HIP_RETURN_NOT_OK(hipMemcpyAsync(&valid_count, d_counter, 8, hipMemcpyDeviceToHost, st));
  }
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  out_arr->null_count = m - valid_count;
  return Status::OK();
}

bool IsInt32Binary(const arrow::DataType& t) { return t.id() == Type::STRING || t.id() == Type::BINARY; }

Status BinaryTakeExec(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  auto* state = static_cast<ShimState<cp::TakeOptions>*>(ctx->state());
  const ArraySpan& values = batch[0].array;
  const ArraySpan& indices = batch[1].array;
  if (!OnRocm3(values) && !OnRocm(indices)) {
    return RunStock(kFnTake, BinaryOffsetWidth(values.type->id()) == 8 ? g_stock_take_large_bin : g_stock_take_bin, state->stock.get(), ctx, batch, out);
  }
  const int tid = IndexTypeId(*indices.type);
  const bool large = BinaryOffsetWidth(values.type->id()) == 8;
  if (tid < 0 || !(IsInt32Binary(*values.type) || large)) {
    return Status::NotImplemented("arrow_amd: take of ", values.type->ToString(), " by ",
                                  indices.type->ToString(), " on device-resident arrays");
  }
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  ArxBinarySpan dv{};
  ArxSpan di{};
  ARROW_RETURN_NOT_OK(DeviceBinarySpan(values, &dv));
  ARROW_RETURN_NOT_OK(DeviceSpan(indices, &di));
  if (state->options.boundscheck) ARROW_RETURN_NOT_OK(CheckBoundsOnDevice(di, tid, values.length, st));
  ARROW_RETURN_NOT_OK(BinaryTakeOnDevice(dv, di, tid, st, out->array_data().get(), large));
  CountGpu(kFnTake);
  return Status::OK();
}

// BinaryFilterImpl == take(GetTakeIndices(filter)): the indices live in device scratch only
Status BinaryFilterExec(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  auto* state = static_cast<ShimState<cp::FilterOptions>*>(ctx->state());
  const ArraySpan& values = batch[0].array;
  const ArraySpan& filter = batch[1].array;
  if (!OnRocm3(values) && !OnRocm(filter)) {
    return RunStock(kFnFilter, BinaryOffsetWidth(values.type->id()) == 8 ? g_stock_filter_large_bin : g_stock_filter_bin, state->stock.get(), ctx, batch, out);
  }
  const bool large = BinaryOffsetWidth(values.type->id()) == 8;
  if (filter.type->id() != Type::BOOL || !(IsInt32Binary(*values.type) || large)) {
    return Status::NotImplemented("arrow_amd: filter of ", values.type->ToString(), " on device-resident arrays");
  }
  if (filter.length > 0xFFFFFFFFll) {
    return Status::NotImplemented("Filter length exceeds UINT32_MAX, consider a different strategy for selecting elements");
  }
  const int null_sel = state->options.null_selection_behavior == cp::FilterOptions::EMIT_NULL
                           ? ARX_FILTER_EMIT_NULL : ARX_FILTER_DROP;
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  ArxBinarySpan dv{};
  ArxSpan dm{};
  ARROW_RETURN_NOT_OK(DeviceBinarySpan(values, &dv));
  ARROW_RETURN_NOT_OK(DeviceSpan(filter, &dm));
  const size_t ws_bytes = arx_filter_workspace_bytes(filter.length);
  void* ws = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kWs, ws_bytes, &ws));
  int64_t out_len = 0;
  ARROW_RETURN_NOT_OK(FromArx(arx_filter_count(&dm, null_sel, ws, ws_bytes, &out_len, st)));
  const bool emit = null_sel == ARX_FILTER_EMIT_NULL && dm.null_count != 0;
  void* d_idx = nullptr;
  void* d_idx_valid = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2, static_cast<size_t>(out_len) * 4 + 64, &d_idx));
  if (emit) ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2Validity, static_cast<size_t>((out_len + 63) / 64) * 8 + 64, &d_idx_valid));
  ARROW_RETURN_NOT_OK(FromArx(arx_mask_to_indices(&dm, null_sel, ws, out_len, 4, d_idx, d_idx_valid, st)));
  ArxSpan di{d_idx_valid, d_idx, 0, out_len, emit ? arrow::kUnknownNullCount : 0};
  ARROW_RETURN_NOT_OK(BinaryTakeOnDevice(dv, di, ARX_UINT32, st, out->array_data().get(), large));
  CountGpu(kFnFilter);
  return Status::OK();
}

// ---------------------------------------------------------------- take
StockKernel g_stock_take;

arrow::Result<std::unique_ptr<cp::KernelState>> TakeInit(cp::KernelContext* ctx,
                                                         const cp::KernelInitArgs& args) {
  auto state = std::make_unique<ShimState<cp::TakeOptions>>();
  if (g_stock_take.init) {
    ARROW_ASSIGN_OR_RAISE(state->stock, g_stock_take.init(ctx, args));
  }
  if (args.options != nullptr) state->options = *static_cast<const cp::TakeOptions*>(args.options);
  return state;
}

int IndexTypeId(const arrow::DataType& t) {
  switch (t.id()) {
    case Type::UINT8: return ARX_UINT8;
    case Type::INT8: return ARX_INT8;
    case Type::UINT16: return ARX_UINT16;
    case Type::INT16: return ARX_INT16;
    case Type::UINT32: return ARX_UINT32;
    case Type::INT32: return ARX_INT32;
    case Type::UINT64: return ARX_UINT64;
    case Type::INT64: return ARX_INT64;
    default: return -1;
  }
}

// FixedWidthTakeExec (vector_selection_take_internal.cc:405-468) with the gather on the GPU.
Status TakeExec(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  auto* state = static_cast<ShimState<cp::TakeOptions>*>(ctx->state());
  const ArraySpan& values = batch[0].array;
  const ArraySpan& indices = batch[1].array;
  const int w = FixedByteWidth(*values.type);
  const int tid = IndexTypeId(*indices.type);
  static const int kIdxWidth[8] = {1, 1, 2, 2, 4, 4, 8, 8};
  if (OnRocm(values) || OnRocm(indices)) {
    if (values.type->id() == Type::BOOL && tid >= 0) {
      hipStream_t st;
      ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
      ArxSpan dv{}, di{};
      ARROW_RETURN_NOT_OK(DeviceSpan(values, &dv));
      ARROW_RETURN_NOT_OK(DeviceSpan(indices, &di));
      if (state->options.boundscheck) ARROW_RETURN_NOT_OK(CheckBoundsOnDevice(di, tid, values.length, st));
      ARROW_RETURN_NOT_OK(BooleanTakeOnDevice(dv, di, tid, st, out->array_data().get()));
      CountGpu(kFnTake);
      return Status::OK();
    }
    if (w == 0 || tid < 0) {
      return Status::NotImplemented("arrow_amd: take of ", values.type->ToString(), " by ",
                                    indices.type->ToString(), " on device-resident arrays");
    }
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    ArxSpan dv{}, di{};
    ARROW_RETURN_NOT_OK(DeviceSpan(values, &dv));
    ARROW_RETURN_NOT_OK(DeviceSpan(indices, &di));
    if (state->options.boundscheck) ARROW_RETURN_NOT_OK(CheckBoundsOnDevice(di, tid, values.length, st));
    const int64_t m = indices.length;
    const bool allocate_validity = dv.null_count != 0 || di.null_count != 0;
    ArrayData* out_arr = out->array_data().get();
    out_arr->length = m;
    out_arr->buffers.resize(2);
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice(m * w));
    out_arr->buffers[0] = nullptr;
    void* d_valid = nullptr;
    void* d_counter = nullptr;
    if (allocate_validity) {
      ARROW_ASSIGN_OR_RAISE(out_arr->buffers[0], AllocDevice(((m + 63) / 64) * 8));
      d_valid = reinterpret_cast<void*>(out_arr->buffers[0]->mutable_address());
      ARROW_RETURN_NOT_OK(t_scratch.Get(kCounter, 64, &d_counter));
      HIP_RETURN_NOT_OK(hipMemsetAsync(d_counter, 0, 8, st));
    }
    ARROW_RETURN_NOT_OK(FromArx(arx_take(&dv, w, &di, tid,
                                         reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address()), d_valid,
                                         static_cast<int64_t*>(d_counter), st)));
    int64_t valid_count = m;
    if (allocate_validity) {
      HIP_RETURN_NOT_OK(hipMemcpyAsync(&valid_count, d_counter, 8, hipMemcpyDeviceToHost, st));
    }
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    out_arr->null_count = m - valid_count;
    CountGpu(kFnTake);
    return Status::OK();
  }
  if (w == 0 || tid < 0 || indices.length < g_min_rows.load() || !IsHost(values) || !IsHost(indices)) {
    return RunStock(kFnTake, g_stock_take, state->stock.get(), ctx, batch, out);
  }
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  ArxSpan dv{}, di{};
  ARROW_RETURN_NOT_OK(Upload(values, w, kValues, kValidity, st, &dv));
  ARROW_RETURN_NOT_OK(Upload(indices, kIdxWidth[tid], kArg2, kArg2Validity, st, &di));
  if (state->options.boundscheck) ARROW_RETURN_NOT_OK(CheckBoundsOnDevice(di, tid, values.length, st));
  const int64_t m = indices.length;
  const bool allocate_validity = values.MayHaveNulls() || indices.MayHaveNulls();
  ArrayData* out_arr = out->array_data().get();
  out_arr->length = m;
  out_arr->buffers.resize(2);
  ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], ctx->Allocate(m * w));
  void* d_out = nullptr;
  void* d_out_valid = nullptr;
  void* d_counter = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kOutData, static_cast<size_t>(m) * w + 16, &d_out));
  if (allocate_validity) {
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[0], ctx->AllocateBitmap(m));
    ARROW_RETURN_NOT_OK(t_scratch.Get(kOutValidity, static_cast<size_t>((m + 63) / 64) * 8 + 16, &d_out_valid));
    ARROW_RETURN_NOT_OK(t_scratch.Get(kCounter, 64, &d_counter));
    HIP_RETURN_NOT_OK(hipMemsetAsync(d_counter, 0, 8, st));
  } else {
    out_arr->buffers[0] = nullptr;
  }
  ARROW_RETURN_NOT_OK(FromArx(arx_take(&dv, w, &di, tid, d_out, d_out_valid,
                                       static_cast<int64_t*>(d_counter), st)));
  HIP_RETURN_NOT_OK(hipMemcpyAsync(out_arr->buffers[1]->mutable_data(), d_out, static_cast<size_t>(m) * w,
                                   hipMemcpyDeviceToHost, st));
  int64_t valid_count = m;
  if (allocate_validity) {
    HIP_RETURN_NOT_OK(hipMemcpyAsync(out_arr->buffers[0]->mutable_data(), d_out_valid,
                                     static_cast<size_t>(arrow::bit_util::BytesForBits(m)),
                                     hipMemcpyDeviceToHost, st));
    HIP_RETURN_NOT_OK(hipMemcpyAsync(&valid_count, d_counter, 8, hipMemcpyDeviceToHost, st));
  }
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  out_arr->null_count = m - valid_count;
  CountGpu(kFnTake);
  return Status::OK();
}

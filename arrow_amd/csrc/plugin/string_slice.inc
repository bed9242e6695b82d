// binary_length / utf8_length / binary_slice / utf8_slice_codeunits on device-resident arrays (csrc/string_slice.hip).
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- string lengths and slices
// One twin per function and input type: binary_length of utf8 / binary (int32) and large_utf8 / large_binary (int64),
// utf8_length of utf8 / large_utf8, binary_slice of binary / large_binary, utf8_slice_codeunits of utf8 / large_utf8.
// A device-resident array runs arx_string_length, or arx_string_slice_offsets + arx_string_slice_data, into HBM
// buffers; the result's validity is the input's, copied to offset 0, and there is no bitmap when the input has none.
// A host batch runs the reference's exec: the length kernels behind the executor's preallocation contract
// (RunStockPrepared), the slice kernels, whose result is a variable-length column, behind RunStockVarLength with the
// null_handling / mem_allocation read off the reference's kernel.  The slice twins run the reference's init first (its
// state serves host batches and its checks stay its own) and keep a copy of SliceOptions for the device call; step 0 is
// the Invalid the reference's exec returns, any other step but 1 has no device kernel and is refused by name.  fixed_size_binary gets no twin: the
// device guard refuses it.
struct StringSliceFunction {
  const char* name;
  int unit;      // ARX_STRING_UNIT_*
  bool slice;
  bool binary;   // takes binary / large_binary
  bool utf8;     // takes utf8 / large_utf8
  Fn fn;
};
const StringSliceFunction kStringSliceFunctions[] = {
    {"binary_length", ARX_STRING_UNIT_BYTES, false, true, true, kFnBinaryLength},
    {"utf8_length", ARX_STRING_UNIT_CODEPOINTS, false, false, true, kFnUtf8Length},
    {"binary_slice", ARX_STRING_UNIT_BYTES, true, true, false, kFnBinarySlice},
    {"utf8_slice_codeunits", ARX_STRING_UNIT_CODEPOINTS, true, false, true, kFnUtf8SliceCodeunits}};

struct StringSliceKernelData : public cp::KernelState {
  const StringSliceFunction* f = nullptr;
  cp::ArrayKernelExec stock_exec = nullptr;
  cp::KernelInit stock_init;   // the slices': the reference's SliceOptions state
  StockContract contract;      // what the executor prepares for the reference's kernel
};

struct DeviceSliceState : public cp::KernelState {
  std::unique_ptr<cp::KernelState> stock;
  cp::SliceOptions options;
};

const StringSliceKernelData* StringSliceDataOf(const cp::Kernel* k) {
  return k != nullptr ? dynamic_cast<const StringSliceKernelData*>(k->data.get()) : nullptr;
}

arrow::Result<std::unique_ptr<cp::KernelState>> StringSliceInit(cp::KernelContext* ctx, const cp::KernelInitArgs& args) {
  const StringSliceKernelData* data = StringSliceDataOf(args.kernel);
  if (data == nullptr || !data->stock_init) return Status::Invalid("arrow_amd: a string slice kernel was initialised without its data");
  auto state = std::make_unique<DeviceSliceState>();
  ARROW_ASSIGN_OR_RAISE(state->stock, data->stock_init(ctx, args));   // the reference's state and its option checks
  if (args.options == nullptr) return Status::Invalid("arrow_amd: ", data->f->name, " without SliceOptions");
  state->options = *static_cast<const cp::SliceOptions*>(args.options);
  return state;
}

// the input's validity at offset 0 into out_arr->buffers[0] (none when it has no nulls) and its null count
Status CopyInputValidity(const ArxBinarySpan& vs, int64_t n, hipStream_t st, ArrayData* out_arr) {
  out_arr->null_count = 0;
  if (vs.validity == nullptr || vs.null_count == 0) return Status::OK();
  ARROW_ASSIGN_OR_RAISE(auto valid, AllocDevice(BitmapBytes(n)));
  ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy(vs.validity, vs.offset, n, reinterpret_cast<void*>(valid->mutable_address()), st)));
  if (vs.null_count > 0) {
    out_arr->null_count = vs.null_count;
  } else {
    ARROW_ASSIGN_OR_RAISE(out_arr->null_count, DeviceNullCount(*valid, n, st));
  }
  if (out_arr->null_count != 0) out_arr->buffers[0] = valid;
  return Status::OK();
}

Status StringSliceExecNP(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  const StringSliceKernelData* kd = StringSliceDataOf(ctx->kernel());
  if (kd == nullptr || kd->stock_exec == nullptr) return Status::Invalid("arrow_amd: a string length / slice kernel ran without its data");
  const StringSliceFunction& f = *kd->f;
  auto* state = f.slice ? static_cast<DeviceSliceState*>(ctx->state()) : nullptr;
  if (f.slice && state == nullptr) return Status::Invalid("arrow_amd: ", f.name, " ran without its state");
  const Type::type in_id = batch[0].type()->id();
  const int offset_width = (in_id == Type::LARGE_STRING || in_id == Type::LARGE_BINARY) ? 8 : 4;
  if (!batch[0].is_array() || !SpanTouchesRocm(batch[0].array)) {
    // ---- a host batch (or a scalar): what the executor would have prepared, then the reference's exec
    if (f.slice) return RunStockVarLength(f.fn, kd->stock_exec, state->stock.get(), kd->contract, ctx, batch, out);
    return RunStockPrepared(f.fn, kd->stock_exec, std::nullopt, offset_width, TwinValidity::kIntersection, ctx, batch, out);
  }
  if (f.slice && state->options.step == 0) return Status::Invalid("Slice step cannot be zero");   // (the reference's exec says so)
  if (f.slice && state->options.step != 1) {
    return Status::NotImplemented("arrow_amd: ", f.name, " with step=", state->options.step,
                                  " on device-resident arrays: only step=1 has a device kernel");
  }
  const ArraySpan& rows = batch[0].array;
  const int64_t n = rows.length;
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  ArxBinarySpan vs{};
  ARROW_RETURN_NOT_OK(DeviceBinarySpan(rows, &vs));
  const int64_t hint = rows.buffers[2].size;
  ArrayData* out_arr = out->array_data().get();
  out_arr->length = n;
  out_arr->offset = 0;
  if (!f.slice) {
    out_arr->buffers.assign(2, nullptr);
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice(std::max<int64_t>(n * offset_width, 8)));
    ARROW_RETURN_NOT_OK(FromArx(arx_string_length(&vs, offset_width, f.unit, hint, ARX_STRING_PATH_AUTO,
                                                  reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address()), st)));
  } else {
    out_arr->buffers.assign(3, nullptr);
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice((n + 1) * offset_width));
    const size_t ws_bytes = arx_string_slice_workspace_bytes(n, offset_width);
    void* ws = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(kBinWs, ws_bytes, &ws));
    void* d_off = reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address());
    int64_t total = 0;
    ARROW_RETURN_NOT_OK(FromArx(arx_string_slice_offsets(&vs, offset_width, f.unit, state->options.start, state->options.stop, hint,
                                                         ARX_STRING_PATH_AUTO, ws, ws_bytes, d_off, &total, st)));
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[2], AllocDevice(std::max<int64_t>(total, 8)));
    ARROW_RETURN_NOT_OK(FromArx(arx_string_slice_data(&vs, offset_width, ws, ws_bytes, d_off, total,
                                                      reinterpret_cast<void*>(out_arr->buffers[2]->mutable_address()), st)));
  }
  ARROW_RETURN_NOT_OK(CopyInputValidity(vs, n, st, out_arr));
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (this thread's scratch may be released after return)
  CountGpu(f.fn);
  return Status::OK();
}

// one twin per function and input type of the table above, appended after the reference's kernels (dispatch takes the
// last match); the reference's own kernels stay behind the device guard (plugin/device_guard.inc)
Status RegisterStringSlice(cp::FunctionRegistry* reg) {
  for (const StringSliceFunction& f : kStringSliceFunctions) {
    std::vector<ValueType> types;
    if (f.utf8) types.insert(types.end(), {ValueType(arrow::utf8()), ValueType(arrow::large_utf8())});
    if (f.binary) types.insert(types.end(), {ValueType(arrow::binary()), ValueType(arrow::large_binary())});
    const StringSliceFunction* fp = &f;
    ARROW_RETURN_NOT_OK(AppendTwins(
        reg, f.name, types, [](const auto& t) { return std::vector<arrow::TypeHolder>{t}; },
        [fp](const ValueType& vt, cp::ScalarKernel* twin) -> arrow::Result<bool> {
          if (twin->data != nullptr || static_cast<bool>(twin->init) != fp->slice) {
            return Status::Invalid("arrow_amd: the reference's ", fp->name, " kernel of ", vt.probe->ToString(), " is not of the expected shape");
          }
          auto data = std::make_shared<StringSliceKernelData>();
          data->f = fp;
          data->stock_exec = twin->exec;
          data->stock_init = twin->init;
          data->contract.null_handling = twin->null_handling;
          data->contract.mem_allocation = twin->mem_allocation;
          twin->data = std::move(data);
          twin->signature = cp::KernelSignature::Make({vt.match}, twin->signature->out_type());
          if (fp->slice) twin->init = StringSliceInit;
          twin->exec = StringSliceExecNP;
          twin->can_write_into_slices = false;
          return true;
        }));
  }
  return Status::OK();
}

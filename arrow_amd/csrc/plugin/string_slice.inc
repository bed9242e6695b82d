// binary_length / utf8_length / binary_slice / utf8_slice_codeunits on device-resident arrays (csrc/string_slice.hip).
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- string lengths and slices
// One twin per function and input type: binary_length of utf8 / binary (int32) and large_utf8 / large_binary (int64),
// utf8_length of utf8 / large_utf8, binary_slice of binary / large_binary, utf8_slice_codeunits of utf8 / large_utf8.
// A device-resident array runs arx_string_length, or arx_string_slice_offsets through SubRangeResultOnDevice
// (plugin/twin.inc), into HBM buffers; the result's validity is the input's (CopyInputValidity).  A host batch runs the
// reference's exec: the length kernels behind the executor's preallocation contract (RunStockPrepared), the slice
// kernels, whose result is a variable-length column, behind RunStockVarLength.  The slice twins keep SliceOptions
// (TwinInit); step 0 is the Invalid the reference's exec returns, any other step but 1 has no device kernel and is
// refused by name.  fixed_size_binary gets no twin: the device guard refuses it.
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

struct StringSliceKernelData : public TwinData {
  const StringSliceFunction* f = nullptr;
};

Status StringSliceExecNP(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  const auto* kd = TwinDataOf<StringSliceKernelData>(ctx->kernel());
  if (kd == nullptr) return TwinWithoutData();
  const StringSliceFunction& f = *kd->f;
  auto* state = f.slice ? static_cast<ShimState<cp::SliceOptions>*>(ctx->state()) : nullptr;
  if (f.slice && state == nullptr) return Status::Invalid("arrow_amd: ", f.name, " ran without its state");
  const int offset_width = BinaryOffsetWidth(batch[0].type()->id());
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
  if (f.slice) {
    const cp::SliceOptions& o = state->options;
    return SubRangeResultOnDevice(
        f.fn, vs, offset_width, st,
        [&](const ArxBinarySpan* v, int width, void* ws, size_t ws_bytes, void* d_off, int64_t* total, hipStream_t s) {
          return arx_string_slice_offsets(v, width, f.unit, o.start, o.stop, hint, ARX_STRING_PATH_AUTO, ws, ws_bytes, d_off, total, s);
        },
        out_arr);
  }
  out_arr->length = n;
  out_arr->offset = 0;
  out_arr->buffers.assign(2, nullptr);
  ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice(std::max<int64_t>(n * offset_width, 8)));
  ARROW_RETURN_NOT_OK(FromArx(arx_string_length(&vs, offset_width, f.unit, hint, ARX_STRING_PATH_AUTO,
                                                reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address()), st)));
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
          auto data = std::make_shared<StringSliceKernelData>();
          data->f = fp;
          ARROW_RETURN_NOT_OK(InstallTwin(fp->name, vt, twin, static_cast<bool>(twin->init) == fp->slice, std::move(data), fp->fn,
                                          TwinInit<cp::SliceOptions, /*kRequired=*/true>, StringSliceExecNP));
          return true;
        }));
  }
  return Status::OK();
}

// match_substring / starts_with / ends_with on device-resident arrays (csrc/match_substring.hip).
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- substring predicates
// The reference's kernels (kernels/scalar_string_ascii.cc: MatchSubstring with the Plain*Matcher of each function) keep
// MatchSubstringOptions in their state.  The added kernels — one per type: utf8, binary, large_utf8, large_binary — keep
// a copy of the options beside the reference's state (TwinInit, plugin/twin.inc).  The pattern goes to the device on the
// first device-resident batch (an init cannot know where the batches will live), once per kernel state: an Acero filter
// reuses it for every batch.  Outputs stay in HBM: the bitmap of matches, and the input's validity
// (CopyInputValidity).  ignore_case has no device kernel: a Status, not a CPU read
// of device memory.  Host batches run the reference's exec on buffers allocated here (the reference's kernels are
// INTERSECTION / PREALLOCATE: the executor would have handed them the input's validity and a values bitmap).
struct MatchSubstringKernelData : public TwinData {
  int op = ARX_MATCH_SUBSTRING;   // ARX_MATCH_*
};

struct DeviceMatchSubstringState : public ShimState<cp::MatchSubstringOptions> {
  std::mutex mu;
  bool uploaded = false;
  std::shared_ptr<Buffer> pattern;   // options.pattern on the device
};

// a host batch (or a scalar): the reference's exec on the buffers the executor would have preallocated for it
Status MatchSubstringStock(cp::KernelContext* ctx, const MatchSubstringKernelData& kd, DeviceMatchSubstringState* s,
                           const cp::ExecSpan& batch, cp::ExecResult* out) {
  ARROW_RETURN_NOT_OK(RunStockPrepared(kd.fn, kd.stock_exec, s->stock.get(), 0, TwinValidity::kIntersection, ctx, batch, out));
  ArrayData* out_arr = out->array_data().get();
  if (out_arr->null_count < 0) {   // (this twin reports an exact count)
    out_arr->null_count = batch.length - arrow::internal::CountSetBits(out_arr->buffers[0]->data(), 0, batch.length);
  }
  return Status::OK();
}

Status MatchSubstringExec(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  const auto* kd = TwinDataOf<MatchSubstringKernelData>(ctx->kernel());
  auto* s = static_cast<DeviceMatchSubstringState*>(ctx->state());
  if (kd == nullptr || s == nullptr) return Status::Invalid("arrow_amd: substring kernel ran without its data or state");
  if (!batch[0].is_array() || !SpanTouchesRocm(batch[0].array)) return MatchSubstringStock(ctx, *kd, s, batch, out);
  if (s->options.ignore_case) {
    return Status::NotImplemented("arrow_amd: ", kFnNames[kd->fn], " with ignore_case on device-resident arrays");
  }
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  const int64_t m = static_cast<int64_t>(s->options.pattern.size());
  {
    std::lock_guard<std::mutex> lock(s->mu);
    if (!s->uploaded) {
      ARROW_ASSIGN_OR_RAISE(s->pattern, AllocDevice(std::max<int64_t>(m, 1)));
      if (m > 0) {
        HIP_RETURN_NOT_OK(hipMemcpyAsync(reinterpret_cast<void*>(s->pattern->mutable_address()), s->options.pattern.data(),
                                         static_cast<size_t>(m), hipMemcpyHostToDevice, st));
        HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (other threads' streams read it next)
      }
      s->uploaded = true;
    }
  }
  const ArraySpan& rows = batch[0].array;
  const int64_t n = rows.length;
  const int offset_width = BinaryOffsetWidth(rows.type->id());
  ArxBinarySpan vs{};
  ARROW_RETURN_NOT_OK(DeviceBinarySpan(rows, &vs));
  ArrayData* out_arr = out->array_data().get();
  out_arr->buffers.assign(2, nullptr);
  ARROW_ASSIGN_OR_RAISE(auto bits, AllocDevice(BitmapBytes(n)));
  ARROW_RETURN_NOT_OK(FromArx(arx_match_substring(&vs, offset_width, kd->op, reinterpret_cast<const void*>(s->pattern->address()), m,
                                                  rows.buffers[2].size, ARX_MATCH_PATH_AUTO,
                                                  reinterpret_cast<void*>(bits->mutable_address()), st)));
  out_arr->buffers[1] = bits;
  ARROW_RETURN_NOT_OK(CopyInputValidity(vs, n, st, out_arr));
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (this thread's scratch may be released after return)
  CountGpu(kd->fn);
  return Status::OK();
}

// the added kernels: one per type, appended after the reference's (dispatch takes the last match); the reference's own
// kernels stay behind the device guard (plugin/device_guard.inc)
Status RegisterMatchSubstring(cp::FunctionRegistry* reg, const char* name, int op, Fn fn_id) {
  return AppendTwins(reg, name, {arrow::utf8(), arrow::binary(), arrow::large_utf8(), arrow::large_binary()},
                     [](const auto& t) { return std::vector<arrow::TypeHolder>{t}; },
                     [=](const ValueType& vt, cp::ScalarKernel* twin) -> arrow::Result<bool> {
                       auto data = std::make_shared<MatchSubstringKernelData>();
                       data->op = op;
                       ARROW_RETURN_NOT_OK(InstallTwin(name, vt, twin, static_cast<bool>(twin->init), std::move(data), fn_id,
                                                       TwinInit<cp::MatchSubstringOptions, /*kRequired=*/true, DeviceMatchSubstringState>,
                                                       MatchSubstringExec));
                       return true;
                     });
}

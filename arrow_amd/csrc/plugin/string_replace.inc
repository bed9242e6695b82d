// replace_substring on device-resident utf8 / binary arrays and their large forms (csrc/string_replace.hip).
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- replace_substring
// One twin per input type: utf8, binary, large_utf8, large_binary (the reference's ReplaceSubstring with the
// PlainSubstringReplacer, kernels/scalar_string_ascii.cc).  A device-resident array runs arx_replace_substring_offsets and
// arx_replace_substring_data through VarLengthResultOnDevice (plugin/twin.inc); a host batch (or a scalar) runs the
// reference's exec behind RunStockVarLength.  The twin keeps a copy of ReplaceSubstringOptions (TwinInit); pattern and
// replacement go to this thread's device scratch on every device call.  The empty pattern has no device kernel (the
// reference does not terminate on it with unlimited replacements) and is refused by name.  replace_substring_regex gets
// no twin: its kernels are the reference's behind the device guard (plugin/device_guard.inc).
Status ReplaceSubstringExecNP(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  const auto* kd = TwinDataOf(ctx->kernel());
  auto* state = static_cast<ShimState<cp::ReplaceSubstringOptions>*>(ctx->state());
  if (kd == nullptr) return TwinWithoutData();
  if (state == nullptr) return Status::Invalid("arrow_amd: replace_substring ran without its state");
  if (!batch[0].is_array() || !SpanTouchesRocm(batch[0].array)) {
    // ---- a host batch (or a scalar): what the executor would have prepared, then the reference's exec
    return RunStockVarLength(kd->fn, kd->stock_exec, state->stock.get(), kd->contract, ctx, batch, out);
  }
  const std::string& pattern = state->options.pattern;
  const std::string& replacement = state->options.replacement;
  if (pattern.empty()) {
    return Status::NotImplemented("arrow_amd: replace_substring with an empty pattern on device-resident arrays: there is no device kernel");
  }
  const int64_t m = static_cast<int64_t>(pattern.size()), r = static_cast<int64_t>(replacement.size());
  const int64_t cap = state->options.max_replacements;
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  void* literals = nullptr;   // pattern, then replacement
  ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2, static_cast<size_t>(m + r), &literals));
  HIP_RETURN_NOT_OK(hipMemcpyAsync(literals, pattern.data(), static_cast<size_t>(m), hipMemcpyHostToDevice, st));
  const void* d_rep = static_cast<const uint8_t*>(literals) + m;
  if (r > 0) HIP_RETURN_NOT_OK(hipMemcpyAsync(const_cast<void*>(d_rep), replacement.data(), static_cast<size_t>(r), hipMemcpyHostToDevice, st));
  ArxBinarySpan vs{};
  ARROW_RETURN_NOT_OK(DeviceBinarySpan(batch[0].array, &vs));
  const int64_t hint = batch[0].array.buffers[2].size;
  const int width = BinaryOffsetWidth(batch[0].type()->id());
  return VarLengthResultOnDevice(
      kd->fn, vs, width, st, arx_replace_substring_workspace_bytes(vs.length, width),
      [&](const ArxBinarySpan* v, int w, void* ws, size_t ws_bytes, void* d_off, int64_t* total, hipStream_t s) {
        return arx_replace_substring_offsets(v, w, literals, m, r, cap, hint, ARX_REPLACE_PATH_AUTO, ws, ws_bytes, d_off, total, s);
      },
      [&](const ArxBinarySpan* v, int w, const void* ws, size_t ws_bytes, const void* d_off, int64_t total, void* d_data, hipStream_t s) {
        return arx_replace_substring_data(v, w, literals, m, d_rep, r, cap, ARX_REPLACE_PATH_AUTO, ws, ws_bytes, d_off, total, d_data, s);
      },
      out->array_data().get());
}

// the twins, appended after the reference's kernels (dispatch takes the last match); the reference's own kernels stay
// behind the device guard (plugin/device_guard.inc)
Status RegisterStringReplace(cp::FunctionRegistry* reg) {
  const std::vector<ValueType> types = {ValueType(arrow::utf8()), ValueType(arrow::binary()), ValueType(arrow::large_utf8()),
                                        ValueType(arrow::large_binary())};
  return AppendTwins(
      reg, kFnNames[kFnReplaceSubstring], types, [](const auto& t) { return std::vector<arrow::TypeHolder>{t}; },
      [](const ValueType& vt, cp::ScalarKernel* twin) -> arrow::Result<bool> {
        ARROW_RETURN_NOT_OK(InstallTwin(kFnNames[kFnReplaceSubstring], vt, twin, static_cast<bool>(twin->init), std::make_shared<TwinData>(),
                                        kFnReplaceSubstring, TwinInit<cp::ReplaceSubstringOptions, /*kRequired=*/true>,
                                        ReplaceSubstringExecNP));
        return true;
      });
}

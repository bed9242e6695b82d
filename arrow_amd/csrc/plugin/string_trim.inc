// The twelve trim functions on device-resident utf8 / large_utf8 arrays (csrc/string_trim.hip).
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- string trimming
// One twin per function and input type, utf8 (int32 offsets) and large_utf8 (int64): the reference has trim kernels for
// no other type.  A device-resident array runs arx_string_trim_offsets through SubRangeResultOnDevice (plugin/twin.inc),
// as the slices do; a host batch (or a scalar) runs the reference's exec behind RunStockVarLength.  The six functions
// that take TrimOptions keep a copy of them for the device call (TwinInit).  The
// reference reports an invalid UTF-8 `characters` from its exec ("Invalid UTF8 sequence in input"), so the device path
// of the utf8_ functions says the same when it decodes them; more than ARX_TRIM_MAX_CODEPOINTS distinct codepoints have
// no device kernel and are refused by name.
struct StringTrimFunction {
  const char* name;
  int sides;      // ARX_TRIM_LEFT / RIGHT / BOTH
  int set_kind;   // ARX_TRIM_*: BYTES and CODEPOINTS take TrimOptions
  Fn fn;
};
const StringTrimFunction kStringTrimFunctions[] = {
    {"ascii_trim_whitespace", ARX_TRIM_BOTH, ARX_TRIM_ASCII_WHITESPACE, kFnAsciiTrimWhitespace},
    {"ascii_ltrim_whitespace", ARX_TRIM_LEFT, ARX_TRIM_ASCII_WHITESPACE, kFnAsciiLtrimWhitespace},
    {"ascii_rtrim_whitespace", ARX_TRIM_RIGHT, ARX_TRIM_ASCII_WHITESPACE, kFnAsciiRtrimWhitespace},
    {"utf8_trim_whitespace", ARX_TRIM_BOTH, ARX_TRIM_UTF8_WHITESPACE, kFnUtf8TrimWhitespace},
    {"utf8_ltrim_whitespace", ARX_TRIM_LEFT, ARX_TRIM_UTF8_WHITESPACE, kFnUtf8LtrimWhitespace},
    {"utf8_rtrim_whitespace", ARX_TRIM_RIGHT, ARX_TRIM_UTF8_WHITESPACE, kFnUtf8RtrimWhitespace},
    {"ascii_trim", ARX_TRIM_BOTH, ARX_TRIM_BYTES, kFnAsciiTrim},
    {"ascii_ltrim", ARX_TRIM_LEFT, ARX_TRIM_BYTES, kFnAsciiLtrim},
    {"ascii_rtrim", ARX_TRIM_RIGHT, ARX_TRIM_BYTES, kFnAsciiRtrim},
    {"utf8_trim", ARX_TRIM_BOTH, ARX_TRIM_CODEPOINTS, kFnUtf8Trim},
    {"utf8_ltrim", ARX_TRIM_LEFT, ARX_TRIM_CODEPOINTS, kFnUtf8Ltrim},
    {"utf8_rtrim", ARX_TRIM_RIGHT, ARX_TRIM_CODEPOINTS, kFnUtf8Rtrim}};

bool TrimTakesOptions(const StringTrimFunction& f) { return f.set_kind == ARX_TRIM_BYTES || f.set_kind == ARX_TRIM_CODEPOINTS; }

struct StringTrimKernelData : public TwinData {
  const StringTrimFunction* f = nullptr;
};

// the codepoints of `characters` as the reference's UTF8Decode reads them: lead and continuation bits only
arrow::Result<std::vector<uint32_t>> TrimCodepoints(const std::string& characters) {
  std::vector<uint32_t> out;
  for (size_t i = 0; i < characters.size();) {
    const uint8_t lead = static_cast<uint8_t>(characters[i]);
    const int extra = lead < 0x80 ? 0 : (lead >= 0xC0 && lead < 0xE0) ? 1 : (lead >= 0xE0 && lead < 0xF0) ? 2 : (lead >= 0xF0 && lead < 0xF8) ? 3 : -1;
    if (extra < 0 || i + extra >= characters.size()) return Status::Invalid("Invalid UTF8 sequence in input");
    uint32_t v = extra == 0 ? lead : lead & (0xFFu >> (extra + 2));
    for (int j = 1; j <= extra; ++j) {
      const uint8_t x = static_cast<uint8_t>(characters[i + j]);
      if ((x & 0xC0) != 0x80) return Status::Invalid("Invalid UTF8 sequence in input");
      v = (v << 6) | (x & 0x3F);
    }
    out.push_back(v);
    i += 1 + extra;
  }
  return out;
}

Status StringTrimExecNP(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  const auto* kd = TwinDataOf<StringTrimKernelData>(ctx->kernel());
  if (kd == nullptr) return TwinWithoutData();
  const StringTrimFunction& f = *kd->f;
  auto* state = TrimTakesOptions(f) ? static_cast<ShimState<cp::TrimOptions>*>(ctx->state()) : nullptr;
  if (TrimTakesOptions(f) && state == nullptr) return Status::Invalid("arrow_amd: ", f.name, " ran without its state");
  if (!batch[0].is_array() || !SpanTouchesRocm(batch[0].array)) {
    // ---- a host batch (or a scalar): what the executor would have prepared, then the reference's exec
    return RunStockVarLength(f.fn, kd->stock_exec, state != nullptr ? std::optional<cp::KernelState*>(state->stock.get()) : std::nullopt,
                             kd->contract, ctx, batch, out);
  }
  const void* set = nullptr;
  int64_t set_length = 0;
  std::vector<uint32_t> codepoints;
  if (f.set_kind == ARX_TRIM_BYTES) {
    set = state->options.characters.data();
    set_length = static_cast<int64_t>(state->options.characters.size());
  } else if (f.set_kind == ARX_TRIM_CODEPOINTS) {
    ARROW_ASSIGN_OR_RAISE(codepoints, TrimCodepoints(state->options.characters));
    std::vector<uint32_t> distinct = codepoints;
    std::sort(distinct.begin(), distinct.end());
    const size_t count = static_cast<size_t>(std::unique(distinct.begin(), distinct.end()) - distinct.begin());
    if (count > ARX_TRIM_MAX_CODEPOINTS) {
      return Status::NotImplemented("arrow_amd: ", f.name, " with ", count, " distinct characters on device-resident arrays: the device "
                                    "kernel takes up to ", static_cast<int>(ARX_TRIM_MAX_CODEPOINTS));
    }
    set = codepoints.data();
    set_length = static_cast<int64_t>(codepoints.size());
  }
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  ArxBinarySpan vs{};
  ARROW_RETURN_NOT_OK(DeviceBinarySpan(batch[0].array, &vs));
  return SubRangeResultOnDevice(
      f.fn, vs, BinaryOffsetWidth(batch[0].type()->id()), st,
      [&](const ArxBinarySpan* v, int width, void* ws, size_t ws_bytes, void* d_off, int64_t* total, hipStream_t s) {
        return arx_string_trim_offsets(v, width, f.sides, f.set_kind, set, set_length, ws, ws_bytes, d_off, total, s);
      },
      out->array_data().get());
}

// one twin per function of the table above for utf8 and large_utf8, appended after the reference's kernels (dispatch
// takes the last match); the reference's own kernels stay behind the device guard (plugin/device_guard.inc)
Status RegisterStringTrim(cp::FunctionRegistry* reg) {
  const std::vector<ValueType> types = {ValueType(arrow::utf8()), ValueType(arrow::large_utf8())};
  for (const StringTrimFunction& f : kStringTrimFunctions) {
    const StringTrimFunction* fp = &f;
    ARROW_RETURN_NOT_OK(AppendTwins(
        reg, f.name, types, [](const auto& t) { return std::vector<arrow::TypeHolder>{t}; },
        [fp](const ValueType& vt, cp::ScalarKernel* twin) -> arrow::Result<bool> {
          auto data = std::make_shared<StringTrimKernelData>();
          data->f = fp;
          ARROW_RETURN_NOT_OK(InstallTwin(fp->name, vt, twin, static_cast<bool>(twin->init) == TrimTakesOptions(*fp), std::move(data), fp->fn,
                                          TwinInit<cp::TrimOptions, /*kRequired=*/true>, StringTrimExecNP));
          return true;
        }));
  }
  return Status::OK();
}

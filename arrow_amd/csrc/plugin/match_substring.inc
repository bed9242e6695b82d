// match_substring / starts_with / ends_with on device-resident arrays (csrc/match_substring.hip).
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- substring predicates
// The reference's kernels (kernels/scalar_string_ascii.cc: MatchSubstring with the Plain*Matcher of each function) keep
// MatchSubstringOptions in their state.  The added kernels — one per type: utf8, binary, large_utf8, large_binary — run
// the reference's init first, so its state serves host batches and its option errors stay its own, and keep a copy of
// the options.  The pattern goes to the device on the first device-resident batch (an init cannot know where the
// batches will live), once per kernel state: an Acero filter reuses it for every batch.  Outputs stay in HBM: the bitmap
// of matches, and the input's validity copied to offset 0.  ignore_case has no device kernel: a Status, not a CPU read
// of device memory.  Host batches run the reference's exec on buffers allocated here (the reference's kernels are
// INTERSECTION / PREALLOCATE: the executor would have handed them the input's validity and a values bitmap).
struct MatchSubstringKernelData : public cp::KernelState {
  int op = ARX_MATCH_SUBSTRING;   // ARX_MATCH_*; also the index into g_stock_match_substring
  Fn fn = kFnMatchSubstring;
};
// the reference's kernels of match_substring [0] / starts_with [1] / ends_with [2] as registered before the shim's
std::vector<cp::ScalarKernel> g_stock_match_substring[3];

struct DeviceMatchSubstringState : public cp::KernelState {
  std::unique_ptr<cp::KernelState> stock;
  cp::ArrayKernelExec stock_exec = nullptr;
  cp::MatchSubstringOptions options;
  std::mutex mu;
  bool uploaded = false;
  std::shared_ptr<Buffer> pattern;   // options.pattern on the device
};

const MatchSubstringKernelData* MatchSubstringDataOf(const cp::Kernel* k) {
  return k != nullptr ? dynamic_cast<const MatchSubstringKernelData*>(k->data.get()) : nullptr;
}

arrow::Result<std::unique_ptr<cp::KernelState>> MatchSubstringInit(cp::KernelContext* ctx, const cp::KernelInitArgs& args) {
  const MatchSubstringKernelData* data = MatchSubstringDataOf(args.kernel);
  if (data == nullptr) return Status::Invalid("arrow_amd: substring kernel without its data");
  auto state = std::make_unique<DeviceMatchSubstringState>();
  const cp::ScalarKernel* stock = nullptr;
  for (const cp::ScalarKernel& k : g_stock_match_substring[data->op]) {
    if (k.signature->MatchesInputs(args.inputs)) stock = &k;   // (the last match, as DispatchExact picks)
  }
  if (stock == nullptr || !stock->init) {
    return Status::Invalid("arrow_amd: no reference ", kFnNames[data->fn], " kernel for ", args.inputs[0].ToString());
  }
  state->stock_exec = stock->exec;
  ARROW_ASSIGN_OR_RAISE(state->stock, stock->init(ctx, args));   // the reference's state and its option checks
  if (args.options == nullptr) return Status::Invalid("arrow_amd: ", kFnNames[data->fn], " without MatchSubstringOptions");
  state->options = *static_cast<const cp::MatchSubstringOptions*>(args.options);
  return state;
}

// a host batch (or a scalar): the reference's exec on the buffers the executor would have preallocated for it
Status MatchSubstringStock(cp::KernelContext* ctx, const MatchSubstringKernelData& kd, DeviceMatchSubstringState* s,
                           const cp::ExecSpan& batch, cp::ExecResult* out) {
  ARROW_RETURN_NOT_OK(RunStockPrepared(kd.fn, s->stock_exec, s->stock.get(), 0, TwinValidity::kIntersection, ctx, batch, out));
  ArrayData* out_arr = out->array_data().get();
  if (out_arr->null_count < 0) {   // (this twin reports an exact count)
    out_arr->null_count = batch.length - arrow::internal::CountSetBits(out_arr->buffers[0]->data(), 0, batch.length);
  }
  return Status::OK();
}

Status MatchSubstringExec(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  const MatchSubstringKernelData* kd = MatchSubstringDataOf(ctx->kernel());
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
  const Type::type id = rows.type->id();
  const int offset_width = (id == Type::LARGE_STRING || id == Type::LARGE_BINARY) ? 8 : 4;
  ArxBinarySpan vs{};
  ARROW_RETURN_NOT_OK(DeviceBinarySpan(rows, &vs));
  ArrayData* out_arr = out->array_data().get();
  out_arr->buffers.assign(2, nullptr);
  ARROW_ASSIGN_OR_RAISE(auto bits, AllocDevice(BitmapBytes(n)));
  ARROW_RETURN_NOT_OK(FromArx(arx_match_substring(&vs, offset_width, kd->op, reinterpret_cast<const void*>(s->pattern->address()), m,
                                                  rows.buffers[2].size, ARX_MATCH_PATH_AUTO,
                                                  reinterpret_cast<void*>(bits->mutable_address()), st)));
  out_arr->buffers[1] = bits;
  out_arr->null_count = 0;
  if (vs.validity != nullptr && vs.null_count != 0) {
    ARROW_ASSIGN_OR_RAISE(auto valid, AllocDevice(BitmapBytes(n)));
    ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy(vs.validity, vs.offset, n, reinterpret_cast<void*>(valid->mutable_address()), st)));
    if (vs.null_count > 0) {
      out_arr->null_count = vs.null_count;
    } else {
      ARROW_ASSIGN_OR_RAISE(out_arr->null_count, DeviceNullCount(*valid, n, st));
    }
    if (out_arr->null_count != 0) out_arr->buffers[0] = valid;
  }
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (this thread's scratch may be released after return)
  CountGpu(kd->fn);
  return Status::OK();
}

// the added kernels: one per type, appended after the reference's (dispatch takes the last match); the reference's own
// kernels stay behind the device guard (plugin/device_guard.inc)
Status RegisterMatchSubstring(cp::FunctionRegistry* reg, const char* name, int op, Fn fn_id) {
  ARROW_ASSIGN_OR_RAISE(auto fn, reg->GetFunction(name));
  if (fn->kind() != cp::Function::SCALAR) return Status::Invalid(name, " is not a scalar function");
  auto& stock = g_stock_match_substring[op];
  stock.clear();
  for (const cp::ScalarKernel* k : static_cast<cp::ScalarFunction*>(fn.get())->kernels()) stock.push_back(*k);
  return AppendTwins(reg, name, {arrow::utf8(), arrow::binary(), arrow::large_utf8(), arrow::large_binary()},
                     [](const auto& t) { return std::vector<arrow::TypeHolder>{t}; },
                     [=](const ValueType& vt, cp::ScalarKernel* twin) -> arrow::Result<bool> {
                       if (twin->data != nullptr || !twin->init) {
                         return Status::Invalid("arrow_amd: the reference's ", name, " kernel of ", vt.probe->ToString(),
                                                " is not of the expected shape");
                       }
                       auto data = std::make_shared<MatchSubstringKernelData>();
                       data->op = op;
                       data->fn = fn_id;
                       twin->data = std::move(data);
                       twin->signature = cp::KernelSignature::Make({vt.match}, twin->signature->out_type());
                       twin->init = MatchSubstringInit;
                       twin->exec = MatchSubstringExec;
                       return true;
                     });
}

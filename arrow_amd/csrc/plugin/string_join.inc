// binary_join_element_wise on device-resident utf8 / binary arrays and their large forms (csrc/string_join.hip).
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- binary_join_element_wise
// One twin per type on the varargs function: utf8, binary, large_utf8, large_binary (the reference's
// BinaryJoinElementWise, kernels/scalar_string_ascii.cc; every operand, the separator included, is of the one type).  A
// batch with at least one device-resident column runs arx_binary_join_offsets and arx_binary_join_data: the columns are
// spans, valid scalars are literals whose bytes go to this thread's device scratch behind the null replacement, null
// scalars are null literals.  The result stays in HBM at offset 0 with an exact null count, and without a bitmap when
// that is 0.  All-host batches (scalars only included) run the reference's exec behind RunStockVarLength; a mix of
// device-resident and host columns, and more operands than ARX_JOIN_MAX_OPERANDS, are refused by name.  The twin keeps a
// copy of JoinOptions (TwinInit).  Under SKIP a row whose values are all null is the empty string on the device, where
// the reference drops the row (include/arrow_amd.h).  binary_join and binary_repeat get no twin: their kernels are the
// reference's behind the device guard (plugin/device_guard.inc).
Status BinaryJoinElementWiseExecNP(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  const auto* kd = TwinDataOf(ctx->kernel());
  auto* state = static_cast<ShimState<cp::JoinOptions>*>(ctx->state());
  if (kd == nullptr) return TwinWithoutData();
  if (state == nullptr) return Status::Invalid("arrow_amd: binary_join_element_wise ran without its state");
  bool any_device = false, any_host = false;
  for (const cp::ExecValue& v : batch.values) {
    if (!v.is_array()) continue;
    if (SpanTouchesRocm(v.array)) any_device = true;
    else any_host = true;
  }
  if (!any_device) {
    // ---- host columns (or scalars only): what the executor would have prepared, then the reference's exec
    return RunStockVarLength(kd->fn, kd->stock_exec, state->stock.get(), kd->contract, ctx, batch, out);
  }
  const char* name = kFnNames[kd->fn];
  if (any_host) {
    return Status::NotImplemented("arrow_amd: ", name, " of ", batch[0].type()->ToString(), " with host and device-resident columns: "
                                  "every column of a device call lives on the device");
  }
  const int num = batch.num_values();
  if (num > ARX_JOIN_MAX_OPERANDS) {
    return Status::NotImplemented("arrow_amd: ", name, " of ", num, " operands on device-resident arrays: a device call takes ",
                                  static_cast<int>(ARX_JOIN_MAX_OPERANDS), ", the separator included");
  }
  const cp::JoinOptions& options = state->options;
  const int mode = options.null_handling == cp::JoinOptions::SKIP      ? ARX_JOIN_SKIP
                   : options.null_handling == cp::JoinOptions::REPLACE ? ARX_JOIN_REPLACE
                                                                        : ARX_JOIN_EMIT_NULL;
  const int64_t n = batch.length;
  const int width = BinaryOffsetWidth(batch[0].type()->id());
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  // the literals back to back: the null replacement, then every valid scalar's bytes
  std::string blob = options.null_replacement;
  std::vector<ArxJoinOperand> operands(static_cast<size_t>(num));
  std::vector<int64_t> literal_at(static_cast<size_t>(num), 0);
  for (int i = 0; i < num; ++i) {
    ArxJoinOperand& op = operands[static_cast<size_t>(i)];
    op = ArxJoinOperand{};
    if (batch[i].is_array()) {
      op.kind = ARX_JOIN_COLUMN;
      ARROW_RETURN_NOT_OK(DeviceBinarySpan(batch[i].array, &op.column));
    } else if (batch[i].scalar->is_valid) {
      const std::string_view bytes = static_cast<const arrow::BaseBinaryScalar&>(*batch[i].scalar).view();
      op.kind = ARX_JOIN_LITERAL;
      op.literal_length = static_cast<int64_t>(bytes.size());
      literal_at[static_cast<size_t>(i)] = static_cast<int64_t>(blob.size());
      blob.append(bytes);
    } else {
      op.kind = ARX_JOIN_NULL;
    }
  }
  void* literals = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2, blob.size() + 8, &literals));
  if (!blob.empty()) HIP_RETURN_NOT_OK(hipMemcpyAsync(literals, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
  for (int i = 0; i < num; ++i) {
    ArxJoinOperand& op = operands[static_cast<size_t>(i)];
    if (op.kind == ARX_JOIN_LITERAL) op.literal = static_cast<const uint8_t*>(literals) + literal_at[static_cast<size_t>(i)];
  }
  const int64_t r = static_cast<int64_t>(options.null_replacement.size());
  ArrayData* out_arr = out->array_data().get();
  out_arr->length = n;
  out_arr->offset = 0;
  out_arr->buffers.assign(3, nullptr);
  ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice((n + 1) * width));
  ARROW_ASSIGN_OR_RAISE(auto valid, AllocDevice(BitmapBytes(n)));
  const size_t ws_bytes = arx_binary_join_workspace_bytes(n, width);
  void* ws = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kBinWs, ws_bytes, &ws));
  void* d_off = reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address());
  int64_t total = 0, nulls = 0;
  ARROW_RETURN_NOT_OK(FromArx(arx_binary_join_offsets(operands.data(), num, n, width, mode, r, ws, ws_bytes, d_off,
                                                      reinterpret_cast<void*>(valid->mutable_address()), &nulls, &total, st)));
  ARROW_ASSIGN_OR_RAISE(out_arr->buffers[2], AllocDevice(std::max<int64_t>(total, 8)));
  ARROW_RETURN_NOT_OK(FromArx(arx_binary_join_data(operands.data(), num, n, width, mode, r > 0 ? literals : nullptr, r, d_off, total,
                                                   reinterpret_cast<void*>(out_arr->buffers[2]->mutable_address()), st)));
  out_arr->null_count = nulls;
  if (nulls != 0) out_arr->buffers[0] = std::move(valid);
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (the literals and this thread's scratch may be released after return)
  CountGpu(kd->fn);
  return Status::OK();
}

// the twins, appended after the reference's kernels (dispatch takes the last match); the reference's own kernels stay
// behind the device guard (plugin/device_guard.inc)
Status RegisterStringJoin(cp::FunctionRegistry* reg) {
  const std::vector<ValueType> types = {ValueType(arrow::utf8()), ValueType(arrow::binary()), ValueType(arrow::large_utf8()),
                                        ValueType(arrow::large_binary())};
  return AppendTwins(
      reg, kFnNames[kFnBinaryJoinElementWise], types, [](const auto& t) { return std::vector<arrow::TypeHolder>{t, t}; },
      [](const ValueType& vt, cp::ScalarKernel* twin) -> arrow::Result<bool> {
        ARROW_RETURN_NOT_OK(InstallTwin(kFnNames[kFnBinaryJoinElementWise], vt, twin, static_cast<bool>(twin->init), std::make_shared<TwinData>(),
                                        kFnBinaryJoinElementWise, TwinInit<cp::JoinOptions>, BinaryJoinElementWiseExecNP,
                                        cp::KernelSignature::Make({vt.match}, twin->signature->out_type(), /*is_varargs=*/true)));
        return true;
      });
}

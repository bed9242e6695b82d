// coalesce / fill_null on device-resident arrays.
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- coalesce(values, fill) — what fill_null calls
// pyarrow's fill_null(values, fill_value) is coalesce(values, fill_value) (CoalesceFunctor, kernels/scalar_if_else.cc): a
// varargs scalar function with one kernel per type.  The added kernels take every fixed-width type and boolean: two
// operands with a device-resident array among them run arx_coalesce2 (the second operand a device array of the same type
// or a scalar; the result lives in HBM), host operands go to the reference kernel behind the executor's preallocation
// contract (COMPUTED_PREALLOCATE / PREALLOCATE, which a NO_PREALLOCATE twin has to honour itself).  More than two
// operands on the device are refused by name.
Status CoalesceExecNP(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  const int64_t n = batch.length;
  ArrayData* out_arr = out->array_data().get();
  out_arr->buffers.resize(2);
  const arrow::DataType& type = *out_arr->type;
  const int width = type.id() == Type::BOOL ? 0 : FixedByteWidth(type);
  bool any_device = false;
  for (const cp::ExecValue& v : batch.values) any_device = any_device || (v.is_array() && SpanTouchesRocm(v.array));
  if (any_device) {
    if (batch.num_values() != 2 || !batch[0].is_array() || !OnRocm(batch[0].array) || (batch[1].is_array() && !OnRocm(batch[1].array))) {
      return Status::NotImplemented("arrow_amd: coalesce on device-resident arrays takes (device array, device array or scalar)");
    }
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    ArxSpan a{}, b{};
    ARROW_RETURN_NOT_OK(DeviceSpan(batch[0].array, &a));
    const ArxSpan* fill = nullptr;
    uint64_t scalar_bits = 0;
    const void* fill_scalar = nullptr;
    if (batch[1].is_array()) {
      ARROW_RETURN_NOT_OK(DeviceSpan(batch[1].array, &b));
      fill = &b;
    } else if (batch[1].scalar->is_valid) {
      const int64_t got = FixedWidthScalarBytes(*batch[1].scalar, width, &scalar_bits);
      if (got != width) return Status::Invalid("arrow_amd: coalesce: a fill scalar of ", got, " bytes for ", type.ToString());
      fill_scalar = &scalar_bits;
    }
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice(width == 0 ? BitmapBytes(n) : std::max<int64_t>(n * width, 8)));
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[0], AllocDevice(BitmapBytes(n)));
    ARROW_RETURN_NOT_OK(FromArx(arx_coalesce2(width, &a, fill, fill_scalar, n, reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address()),
                                              reinterpret_cast<void*>(out_arr->buffers[0]->mutable_address()), st)));
    const bool no_nulls = n == 0 || fill_scalar != nullptr || a.validity == nullptr || a.null_count == 0;
    if (no_nulls) {   // every slot has a value: no bitmap, like the reference's result
      HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
      out_arr->buffers[0] = nullptr;
      out_arr->null_count = 0;
    } else {
      ARROW_ASSIGN_OR_RAISE(out_arr->null_count, DeviceNullCount(*out_arr->buffers[0], n, st));   // (synchronizes)
    }
    CountGpu(kFnCoalesce);
    return Status::OK();
  }
  // ---- host operands: the executor's preallocation, then the reference kernel
  const TwinData* kd = TwinDataOf(ctx->kernel());
  if (kd == nullptr) return TwinWithoutData();
  return RunStockPrepared(kFnCoalesce, kd->stock_exec, std::nullopt, width, TwinValidity::kAllocate, ctx, batch, out);
}

Status RegisterCoalesce(cp::FunctionRegistry* reg) {
  return AppendTwins(reg, "coalesce", FixedWidthTwinTypes(/*with_decimal128=*/false),
                     [](const auto& t) { return std::vector<arrow::TypeHolder>{t, t}; },
                     [](const ValueType& vt, cp::ScalarKernel* twin) -> arrow::Result<bool> {
                       if (twin->data != nullptr) return false;   // (none of the reference's coalesce kernels carries data)
                       ARROW_RETURN_NOT_OK(InstallTwin("coalesce", vt, twin, true, std::make_shared<TwinData>(), kFnCoalesce, nullptr, CoalesceExecNP,
                                                       cp::KernelSignature::Make({vt.match}, twin->signature->out_type(), /*is_varargs=*/true)));
                       return true;
                     });
}

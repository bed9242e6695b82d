// if_else on device-resident arrays (csrc/if_else.hip).
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- if_else(cond, left, right)
// The reference has one kernel per type (IfElseFunctor, kernels/scalar_if_else.cc; COMPUTED_PREALLOCATE / PREALLOCATE).
// The added kernels take boolean and every fixed-width type up to decimal128: a device-resident boolean cond with
// left / right each a device array of the result's type or a scalar runs arx_if_else (the result lives in HBM, without a
// bitmap when no operand can be null); host operands — scalars and a scalar cond included — go to the reference kernel
// behind the executor's preallocation contract, which a NO_PREALLOCATE twin has to honour itself (as CoalesceExecNP
// does).  A mix of host and device arrays and a scalar cond over device operands are refused by name; device arrays of
// every other type reach the reference's own kernels, which sit behind the device guard (plugin/device_guard.inc).
// left / right of a device call as arx_if_else takes it: *span stays NULL for a scalar, *scalar for an array and a null scalar
Status IfElseOperand(const cp::ExecValue& v, int width, const arrow::DataType& type, ArxSpan* storage, uint8_t* scalar_bytes,
                     const ArxSpan** span, const void** scalar) {
  *span = nullptr;
  *scalar = nullptr;
  if (v.is_array()) {
    ARROW_RETURN_NOT_OK(DeviceSpan(v.array, storage));
    *span = storage;
    return Status::OK();
  }
  if (!v.scalar->is_valid) return Status::OK();
  const int64_t got = FixedWidthScalarBytes(*v.scalar, width, scalar_bytes);
  if (got != width) return Status::Invalid("arrow_amd: if_else: a scalar of ", got, " bytes for ", type.ToString());
  *scalar = scalar_bytes;
  return Status::OK();
}

Status IfElseExecNP(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  const int64_t n = batch.length;
  ArrayData* out_arr = out->array_data().get();
  out_arr->buffers.resize(2);
  const arrow::DataType& type = *out_arr->type;
  const int width = type.id() == Type::BOOL ? 0 : FixedByteWidth(type);
  bool any_device = false, any_host = false;
  for (const cp::ExecValue& v : batch.values) {
    if (!v.is_array()) continue;
    if (SpanTouchesRocm(v.array)) any_device = true;
    else any_host = true;
  }
  if (any_device) {
    if (batch.num_values() != 3 || any_host || !batch[0].is_array()) {
      return Status::NotImplemented("arrow_amd: if_else on device-resident arrays takes (device boolean array, device array or scalar, "
                                    "device array or scalar): ", any_host ? "a mix of host and device arrays" : "a scalar cond",
                                    " is not on the device path");
    }
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    ArxSpan c{}, storage[2] = {};
    ARROW_RETURN_NOT_OK(DeviceSpan(batch[0].array, &c));
    alignas(16) uint8_t scalar_bytes[2][16] = {};
    const ArxSpan* span[2];
    const void* scalar[2];
    bool may_have_nulls = c.validity != nullptr && c.null_count != 0;
    for (int i = 0; i < 2; ++i) {
      ARROW_RETURN_NOT_OK(IfElseOperand(batch[1 + i], width, type, &storage[i], scalar_bytes[i], &span[i], &scalar[i]));
      may_have_nulls = may_have_nulls || (span[i] != nullptr ? (span[i]->validity != nullptr && span[i]->null_count != 0) : scalar[i] == nullptr);
    }
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice(width == 0 ? BitmapBytes(n) : std::max<int64_t>(n * width, 8)));
    out_arr->buffers[0] = nullptr;
    if (may_have_nulls) {
      ARROW_ASSIGN_OR_RAISE(out_arr->buffers[0], AllocDevice(BitmapBytes(n)));
    }
    ARROW_RETURN_NOT_OK(FromArx(arx_if_else(width, &c, span[0], scalar[0], span[1], scalar[1], n,
                                            reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address()),
                                            may_have_nulls ? reinterpret_cast<void*>(out_arr->buffers[0]->mutable_address()) : nullptr, st)));
    if (may_have_nulls) {
      ARROW_ASSIGN_OR_RAISE(out_arr->null_count, DeviceNullCount(*out_arr->buffers[0], n, st));   // (synchronizes)
    } else {   // every slot has a value: no bitmap, like the reference's result
      HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
      out_arr->null_count = 0;
    }
    CountGpu(kFnIfElse);
    return Status::OK();
  }
  // ---- host operands: the executor's preallocation, then the reference kernel
  const TwinData* kd = TwinDataOf(ctx->kernel());
  if (kd == nullptr) return TwinWithoutData();
  return RunStockPrepared(kFnIfElse, kd->stock_exec, std::nullopt, width, TwinValidity::kAllocate, ctx, batch, out);
}

// the result's type is the operands' (the reference's kernel of a probe type may state that very type: time32[s])
arrow::Result<arrow::TypeHolder> ResolveIfElseType(cp::KernelContext*, const std::vector<arrow::TypeHolder>& types) {
  return types.back();
}

Status RegisterIfElse(cp::FunctionRegistry* reg) {
  return AppendTwins(reg, "if_else", FixedWidthTwinTypes(/*with_decimal128=*/true),
                     [](const auto& t) { return std::vector<arrow::TypeHolder>{arrow::boolean(), t, t}; },
                     [](const ValueType& vt, cp::ScalarKernel* twin) -> arrow::Result<bool> {
                       if (twin->data != nullptr) return false;   // (none of the reference's if_else kernels carries data)
                       ARROW_RETURN_NOT_OK(InstallTwin("if_else", vt, twin, true, std::make_shared<TwinData>(), kFnIfElse, nullptr, IfElseExecNP,
                                                       cp::KernelSignature::Make({cp::InputType(arrow::boolean()), vt.match, vt.match},
                                                                                 cp::OutputType(ResolveIfElseType))));
                       return true;
                     });
}

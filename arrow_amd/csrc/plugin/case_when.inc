// case_when on device-resident arrays (csrc/case_when.hip).
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- case_when(cond_struct, v_0 .. v_{k-1} [, else])
// The reference has one varargs kernel per type (CaseWhenFunctor, kernels/scalar_if_else.cc; COMPUTED_PREALLOCATE /
// PREALLOCATE for the fixed-width types).  The added kernels take the types if_else takes: a struct of boolean fields
// whose children are device arrays, with every value a device array of the result's type or a scalar, runs
// arx_case_when (the result lives in HBM, without a bitmap when there is an else and no value can be null); host operands
// go to the reference kernel behind the executor's preallocation contract.  A mix of host and device arrays, a scalar
// cond struct over device values and more than ARX_CASE_WHEN_MAX_CONDS conds are refused by name; device arrays of every
// other type reach the reference's own kernels, which sit behind the device guard (plugin/device_guard.inc).  The two
// argument checks the reference makes ahead of its loop keep its texts.
Status CaseWhenExecNP(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
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
    if (any_host || !batch[0].is_array()) {
      return Status::NotImplemented("arrow_amd: case_when on device-resident arrays takes (struct of device boolean arrays, device arrays "
                                    "or scalars ...): ", any_host ? "a mix of host and device arrays" : "a scalar cond struct",
                                    " is not on the device path");
    }
    const ArraySpan& conds = batch[0].array;
    const int num_conds = static_cast<int>(conds.child_data.size());
    const int num_values = batch.num_values() - 1;
    if (num_values != num_conds && num_values != num_conds + 1) {   // (the reference's check and text)
      return Status::Invalid("case_when: number of struct fields must be equal to or one less than count of remaining arguments (",
                             num_values, "), got: ", num_conds);
    }
    if (num_conds > ARX_CASE_WHEN_MAX_CONDS) {
      return Status::NotImplemented("arrow_amd: case_when with ", num_conds, " conds on device-resident arrays: the device kernel takes up to ",
                                    ARX_CASE_WHEN_MAX_CONDS);
    }
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    // top-level nulls of the struct: a bitmap in HBM is counted on the device unless the struct carries a positive count
    // (an unknown count of a non-CPU bitmap may have been settled as zero before the kernel sees the span)
    const auto* top = conds.buffers[0].owner;
    if (top != nullptr && *top != nullptr) {
      int64_t nulls = conds.null_count;
      if (nulls <= 0) {
        ArxSpan whole{};
        ARROW_RETURN_NOT_OK(DeviceSpan(conds, &whole));
        ARROW_ASSIGN_OR_RAISE(auto packed, AllocDevice(BitmapBytes(n)));
        ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy(whole.validity, whole.offset, n, reinterpret_cast<void*>(packed->mutable_address()), st)));
        ARROW_ASSIGN_OR_RAISE(nulls, DeviceNullCount(*packed, n, st));
      }
      if (nulls != 0) return Status::Invalid("cond struct must not be a null scalar or have top-level nulls");
    }
    ArxSpan cond_spans[ARX_CASE_WHEN_MAX_CONDS] = {};
    const ArxSpan* cond_ptrs[ARX_CASE_WHEN_MAX_CONDS] = {};
    for (int j = 0; j < num_conds; ++j) {
      const ArraySpan& field = conds.child_data[j];
      if (field.type->id() != Type::BOOL) return Status::TypeError("case_when: all fields of the cond struct must be boolean, field ", j, " is ", field.type->ToString());
      ARROW_RETURN_NOT_OK(DeviceSpan(field, &cond_spans[j]));
      // a field carries its own offset on top of the struct's, and may be longer than the struct
      cond_spans[j].offset = field.offset + conds.offset;
      cond_spans[j].length = n;
      if (conds.offset != 0 || field.length != n) cond_spans[j].null_count = field.null_count == 0 ? 0 : arrow::kUnknownNullCount;
      cond_ptrs[j] = &cond_spans[j];
    }
    ArxSpan value_spans[ARX_CASE_WHEN_MAX_CONDS + 1] = {};
    ArxOperand values[ARX_CASE_WHEN_MAX_CONDS + 1] = {};
    alignas(16) uint8_t scalar_bytes[ARX_CASE_WHEN_MAX_CONDS + 1][16] = {};
    bool may_have_nulls = num_values == num_conds;
    for (int j = 0; j < num_values; ++j) {
      ARROW_RETURN_NOT_OK(IfElseOperand(batch[1 + j], width, type, &value_spans[j], scalar_bytes[j], &values[j].span, &values[j].scalar));
      may_have_nulls = may_have_nulls || (values[j].span != nullptr ? (values[j].span->validity != nullptr && values[j].span->null_count != 0)
                                                                    : values[j].scalar == nullptr);
    }
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice(width == 0 ? BitmapBytes(n) : std::max<int64_t>(n * width, 8)));
    out_arr->buffers[0] = nullptr;
    if (may_have_nulls) {
      ARROW_ASSIGN_OR_RAISE(out_arr->buffers[0], AllocDevice(BitmapBytes(n)));
    }
    ARROW_RETURN_NOT_OK(FromArx(arx_case_when(width, cond_ptrs, num_conds, values, num_values, n,
                                              reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address()),
                                              may_have_nulls ? reinterpret_cast<void*>(out_arr->buffers[0]->mutable_address()) : nullptr, st)));
    if (may_have_nulls) {
      ARROW_ASSIGN_OR_RAISE(out_arr->null_count, DeviceNullCount(*out_arr->buffers[0], n, st));   // (synchronizes)
    } else {   // every slot has a value: no bitmap
      HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
      out_arr->null_count = 0;
    }
    CountGpu(kFnCaseWhen);
    return Status::OK();
  }
  // ---- host operands: the executor's preallocation, then the reference kernel
  const TwinData* kd = TwinDataOf(ctx->kernel());
  if (kd == nullptr) return TwinWithoutData();
  return RunStockPrepared(kFnCaseWhen, kd->stock_exec, std::nullopt, width, TwinValidity::kAllocate, ctx, batch, out);
}

Status RegisterCaseWhen(cp::FunctionRegistry* reg) {
  const auto conds = arrow::struct_({arrow::field("c", arrow::boolean())});
  return AppendTwins(reg, "case_when", FixedWidthTwinTypes(/*with_decimal128=*/true),
                     [conds](const auto& t) { return std::vector<arrow::TypeHolder>{conds, t}; },
                     [](const ValueType& vt, cp::ScalarKernel* twin) -> arrow::Result<bool> {
                       if (twin->data != nullptr) return false;   // (none of the reference's case_when kernels carries data)
                       ARROW_RETURN_NOT_OK(InstallTwin("case_when", vt, twin, true, std::make_shared<TwinData>(), kFnCaseWhen, nullptr, CaseWhenExecNP,
                                                       cp::KernelSignature::Make({cp::InputType(Type::STRUCT), vt.match},
                                                                                 cp::OutputType(ResolveIfElseType), /*is_varargs=*/true)));
                       return true;
                     });
}

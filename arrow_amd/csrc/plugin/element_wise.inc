// min_element_wise / max_element_wise on device-resident arrays (csrc/element_wise.hip).
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- min_element_wise / max_element_wise(v_0 .. v_{k-1})
// The reference has one varargs kernel per type (ScalarMinMax, kernels/scalar_compare.cc) with ElementWiseAggregateOptions
// in its state.  The added kernels take the ten numeric types and the temporal types that are physically int32 / int64
// (they run the integer kernels): device arrays, with scalars in any position, run arx_min_max_element_wise (the result
// lives in HBM, without a bitmap when it cannot hold a null); host operands go to the reference kernel with what the
// executor would have prepared for it.  A mix of host and device arrays and more than ARX_ELEMENT_WISE_MAX_OPERANDS
// operands are refused by name; device arrays of every other type reach the reference's own kernels, which sit behind the
// device guard (plugin/device_guard.inc).
struct ElementWiseTwinData : public TwinData {
  int op = ARX_ELEMENT_WISE_MIN;
};

int ElementWiseNumType(const arrow::DataType& t) {
  const int direct = UnaryNumericTypeId(t.id());
  if (direct >= 0) return direct;
  switch (t.id()) {
    case Type::DATE32: case Type::TIME32: return ARX_NUM_INT32;
    case Type::DATE64: case Type::TIME64: case Type::TIMESTAMP: case Type::DURATION: return ARX_NUM_INT64;
    default: return -1;
  }
}

Status ElementWiseExecNP(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  const int64_t n = batch.length;
  ArrayData* out_arr = out->array_data().get();
  out_arr->buffers.resize(2);
  const arrow::DataType& type = *out_arr->type;
  const int width = FixedByteWidth(type);
  const auto* kd = TwinDataOf<ElementWiseTwinData>(ctx->kernel());
  if (kd == nullptr) return TwinWithoutData();
  auto* state = static_cast<ShimState<cp::ElementWiseAggregateOptions>*>(ctx->state());
  bool any_device = false, any_host = false;
  for (const cp::ExecValue& v : batch.values) {
    if (!v.is_array()) continue;
    if (SpanTouchesRocm(v.array)) any_device = true;
    else any_host = true;
  }
  if (any_device) {
    const int num_operands = batch.num_values();
    if (any_host) {
      return Status::NotImplemented("arrow_amd: ", kFnNames[kd->fn], " on device-resident arrays takes device arrays and scalars: a mix of "
                                    "host and device arrays is not on the device path");
    }
    if (num_operands > ARX_ELEMENT_WISE_MAX_OPERANDS) {
      return Status::NotImplemented("arrow_amd: ", kFnNames[kd->fn], " with ", num_operands, " operands on device-resident arrays: the device "
                                    "kernel takes up to ", ARX_ELEMENT_WISE_MAX_OPERANDS);
    }
    const int num_type = ElementWiseNumType(type);
    if (num_type < 0) return Status::NotImplemented("arrow_amd: ", kFnNames[kd->fn], " of ", type.ToString(), " on device-resident arrays");
    const bool skip_nulls = state->options.skip_nulls;
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    ArxSpan spans[ARX_ELEMENT_WISE_MAX_OPERANDS] = {};
    ArxOperand operands[ARX_ELEMENT_WISE_MAX_OPERANDS] = {};
    alignas(16) uint8_t scalar_bytes[ARX_ELEMENT_WISE_MAX_OPERANDS][16] = {};
    bool any_nullable = false, all_nullable = true;
    for (int j = 0; j < num_operands; ++j) {
      ARROW_RETURN_NOT_OK(IfElseOperand(batch[j], width, type, &spans[j], scalar_bytes[j], &operands[j].span, &operands[j].scalar));
      const bool nullable = operands[j].span != nullptr ? (operands[j].span->validity != nullptr && operands[j].span->null_count != 0)
                                                        : operands[j].scalar == nullptr;
      any_nullable = any_nullable || nullable;
      all_nullable = all_nullable && nullable;
    }
    const bool may_have_nulls = skip_nulls ? all_nullable : any_nullable;
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice(std::max<int64_t>(n * width, 8)));
    out_arr->buffers[0] = nullptr;
    if (may_have_nulls) {
      ARROW_ASSIGN_OR_RAISE(out_arr->buffers[0], AllocDevice(BitmapBytes(n)));
    }
    ARROW_RETURN_NOT_OK(FromArx(arx_min_max_element_wise(num_type, kd->op, skip_nulls ? 1 : 0, operands, num_operands, n,
                                                         reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address()),
                                                         may_have_nulls ? reinterpret_cast<void*>(out_arr->buffers[0]->mutable_address()) : nullptr,
                                                         st)));
    if (may_have_nulls) {
      ARROW_ASSIGN_OR_RAISE(out_arr->null_count, DeviceNullCount(*out_arr->buffers[0], n, st));   // (synchronizes)
    } else {   // every slot has a value: no bitmap
      HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
      out_arr->null_count = 0;
    }
    CountGpu(kd->fn);
    return Status::OK();
  }
  // ---- host operands: what the executor prepares for the reference's kernel, read off the kernel's own enums (the data
  // buffer under PREALLOCATE; the kernel makes its own validity under COMPUTED_NO_PREALLOCATE), then the reference's exec
  const TwinValidity policy = kd->contract.null_handling == cp::NullHandling::INTERSECTION           ? TwinValidity::kIntersection
                              : kd->contract.null_handling == cp::NullHandling::COMPUTED_PREALLOCATE ? TwinValidity::kAllocate
                                                                                                     : TwinValidity::kNone;
  PreparedOutput p;
  ARROW_RETURN_NOT_OK(p.PrepareValidity(ctx, batch, policy));
  out_arr->length = n;
  out_arr->offset = 0;
  out_arr->buffers[0] = std::move(p.validity);
  out_arr->null_count = kd->contract.null_handling == cp::NullHandling::COMPUTED_NO_PREALLOCATE ? arrow::kUnknownNullCount : p.null_count;
  if (kd->contract.mem_allocation == cp::MemAllocation::PREALLOCATE) {
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], ctx->Allocate(n * width));
  }
  return RunStock(kd->fn, kd->stock_exec, std::optional<cp::KernelState*>(state->stock.get()), ctx, batch, out);
}

Status RegisterElementWise(cp::FunctionRegistry* reg, const char* name, int op, Fn fn) {
  // the reference's kernels are of exact types: one per unit, and none for a timestamp with a time zone
  std::vector<ValueType> types = {arrow::int8(), arrow::uint8(), arrow::int16(), arrow::uint16(), arrow::int32(), arrow::uint32(),
                                  arrow::int64(), arrow::uint64(), arrow::float32(), arrow::float64(), arrow::date32(), arrow::date64(),
                                  arrow::time32(arrow::TimeUnit::SECOND), arrow::time32(arrow::TimeUnit::MILLI),
                                  arrow::time64(arrow::TimeUnit::MICRO), arrow::time64(arrow::TimeUnit::NANO)};
  for (const auto unit : {arrow::TimeUnit::SECOND, arrow::TimeUnit::MILLI, arrow::TimeUnit::MICRO, arrow::TimeUnit::NANO}) {
    types.push_back(ValueType(arrow::timestamp(unit)));
    types.push_back(ValueType(arrow::duration(unit)));
  }
  return AppendTwins(reg, name, types, [](const auto& t) { return std::vector<arrow::TypeHolder>{t, t}; },
                     [name, op, fn](const ValueType& vt, cp::ScalarKernel* twin) -> arrow::Result<bool> {
                       if (twin->data != nullptr) return false;   // (none of the reference's kernels carries data)
                       auto data = std::make_shared<ElementWiseTwinData>();
                       data->op = op;
                       ARROW_RETURN_NOT_OK(InstallTwin(name, vt, twin, static_cast<bool>(twin->init), std::move(data), fn,
                                                       TwinInit<cp::ElementWiseAggregateOptions>, ElementWiseExecNP,
                                                       cp::KernelSignature::Make({vt.match}, twin->signature->out_type(), /*is_varargs=*/true)));
                       return true;
                     });
}

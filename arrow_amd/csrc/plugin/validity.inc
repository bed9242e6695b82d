// is_valid / is_null / true_unless_null on device-resident arrays.
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- the validity predicates
// IsValidExec / IsNullExec / TrueUnlessNullExec (kernels/scalar_validity.cc:39-61,104-140,245-262) read
// `arr.MayHaveNulls()` and `arr.buffers[0].data`: for a device-resident array the executor's span has neither (the
// validity pointer of a non-CPU buffer is null, so null_count is taken as 0), and the reference answers "no nulls" —
// silently: `filter(is_valid(v))` over a device table would keep the null rows.  These twins compute the predicate on
// the device from the validity bitmap the Buffer owns (arx_bitmap_copy / arx_boolean_invert, or a fill when the array
// has no bitmap) and leave the boolean result in HBM, where the filter kernels want their mask.  Host arrays take the
// reference's exec, given the output it would have been preallocated (MemAllocation::PREALLOCATE; OUTPUT_NOT_NULL for
// is_valid / is_null, INTERSECTION for true_unless_null).  Types whose nulls are not (only) the validity bitmap —
// null, unions, run-end encoded, dictionaries — and is_null(nan_is_null = true) of floating columns are refused by
// name on the device route.
enum ValidityKind { kIsValid = 0, kIsNull, kTrueUnlessNull };

template <int KIND>
Status ValidityExecNP(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  static const char* const kNames[3] = {"is_valid", "is_null", "true_unless_null"};
  const TwinData* kd = TwinDataOf(ctx->kernel());
  if (kd == nullptr) return TwinWithoutData();
  auto* state = static_cast<ShimState<cp::NullOptions>*>(ctx->state());   // (null: the reference's kernel has no init)
  const int64_t n = batch.length;
  ArrayData* out_arr = out->array_data().get();
  out_arr->buffers.resize(2);
  out_arr->buffers[0] = nullptr;
  out_arr->null_count = 0;
  const ArraySpan& a = batch[0].array;
  if (batch[0].is_array() && SpanTouchesRocm(a)) {
    const Type::type id = a.type->id();
    if (id == Type::NA || id == Type::SPARSE_UNION || id == Type::DENSE_UNION || id == Type::RUN_END_ENCODED ||
        id == Type::DICTIONARY) {
      return Status::NotImplemented("arrow_amd: ", kNames[KIND], " of ", a.type->ToString(), " on device-resident arrays (the nulls "
                                    "of this type are not its validity bitmap)");
    }
    if (KIND == kIsNull && state != nullptr && state->options.nan_is_null && arrow::is_floating(id)) {
      return Status::NotImplemented("arrow_amd: is_null(nan_is_null = true) of ", a.type->ToString(), " on device-resident arrays");
    }
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    const int64_t bytes = BitmapBytes(n);
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice(bytes));
    void* d_out = reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address());
    const void* validity = nullptr;
    if (a.buffers[0].owner != nullptr && *a.buffers[0].owner != nullptr) {
      validity = reinterpret_cast<const void*>((*a.buffers[0].owner)->address());
    }
    if (validity == nullptr) {       // no bitmap: every slot is valid
      HIP_RETURN_NOT_OK(hipMemsetAsync(d_out, KIND == kIsNull ? 0 : 0xFF, static_cast<size_t>(bytes), st));
    } else if (KIND == kIsNull) {
      ARROW_RETURN_NOT_OK(FromArx(arx_boolean_invert(validity, a.offset, n, d_out, st)));
    } else if (KIND == kIsValid) {
      ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy(validity, a.offset, n, d_out, st)));
    } else {
      // true_unless_null: all true, null where the input is (NullHandling::INTERSECTION)
      HIP_RETURN_NOT_OK(hipMemsetAsync(d_out, 0xFF, static_cast<size_t>(bytes), st));
      ARROW_ASSIGN_OR_RAISE(out_arr->buffers[0], AllocDevice(bytes));
      ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy(validity, a.offset, n, reinterpret_cast<void*>(out_arr->buffers[0]->mutable_address()), st)));
      if (n > 0) {
        ARROW_ASSIGN_OR_RAISE(out_arr->null_count, DeviceNullCount(*out_arr->buffers[0], n, st));
      }
    }
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    CountGpu(kFnBoolean);
    return Status::OK();
  }
  // host operand: the output the executor would have preallocated, then the reference's exec
  // (is_valid / is_null: OUTPUT_NOT_NULL; true_unless_null: INTERSECTION, where the NullPropagator, exec.cc, answers a null-typed or
  // all-null array with an all-clear bitmap instead of a copy)
  const bool propagate = KIND == kTrueUnlessNull && batch[0].is_array();
  const bool all_null = propagate && (a.type->id() == Type::NA || (n > 0 && a.null_count == n));
  PreparedOutput p;
  ARROW_RETURN_NOT_OK(p.Prepare(ctx, batch, out_arr->type.get(), 0,
                                all_null ? TwinValidity::kAllocate : propagate ? TwinValidity::kIntersection : TwinValidity::kNone));
  if (all_null) p.null_count = p.tmp.array_span_mutable()->null_count = n;
  ARROW_RETURN_NOT_OK(RunStock(kFnBoolean, kd->stock_exec,
                               std::optional<cp::KernelState*>(state != nullptr ? state->stock.get() : nullptr), ctx, batch, &p.tmp));
  p.MoveInto(out_arr);
  return Status::OK();
}

template <int KIND>
Status RegisterValidityNP(cp::FunctionRegistry* reg, const char* name) {
  return AppendTwins(reg, name, {arrow::int64()}, [](const auto& t) { return std::vector<arrow::TypeHolder>{t}; },
                     [name](const ValueType& vt, cp::ScalarKernel* twin) -> arrow::Result<bool> {
                       ARROW_RETURN_NOT_OK(InstallTwin(name, vt, twin, true, std::make_shared<TwinData>(), kFnBoolean, TwinInit<cp::NullOptions>,
                                                       ValidityExecNP<KIND>, twin->signature));   // (the reference's signature stays: any type)
                       return true;
                     });
}

// equal / not_equal / greater / greater_equal / less / less_equal of utf8 / binary columns on device-resident arrays
// (csrc/string_compare.hip).
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- string comparisons
// The reference has one kernel per (function, base binary type) (CompareKernel, kernels/scalar_compare.cc; INTERSECTION /
// PREALLOCATE, no init).  The added kernels — six functions x utf8, binary, large_utf8, large_binary, both operands of
// the one type — take two device arrays, or one device array and a scalar on either side: the scalar's bytes go to the
// device, one arx_compare_binary call writes the answers, the validity is intersected on the device, and the result stays
// in HBM at offset 0 with an exact null count.  A null scalar gives an all-null result without a launch.  Host operands
// run the reference's exec on the buffers the executor would have preallocated; one host and one device array is
// refused by name.
// less / less_equal: the reference builds their kernels as flipped copies of greater / greater_equal, the unflipped
// exec in Kernel::data (MakeFlippedFunction, scalar_compare.cc) — a kernel InstallTwin refuses.  Their twins are made
// from the greater / greater_equal kernel of the same type instead and swap the operands of a host batch themselves.
struct StringCompareKernelData : public TwinData {
  int op = ARX_CMP_EQUAL;        // ARX_CMP_*
  bool swap_for_stock = false;   // stock_exec answers the operands the other way round
};

const char* const kStringCompareNames[6] = {"equal", "not_equal", "greater", "greater_equal", "less", "less_equal"};

Status StringCompareExec(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  const auto* kd = TwinDataOf<StringCompareKernelData>(ctx->kernel());
  if (kd == nullptr) return TwinWithoutData();
  const char* name = kStringCompareNames[kd->op];
  bool any_device = false, any_host = false;
  for (const cp::ExecValue& v : batch.values) {
    if (!v.is_array()) continue;
    if (SpanTouchesRocm(v.array)) any_device = true;
    else any_host = true;
  }
  ArrayData* out_arr = out->array_data().get();
  if (!any_device) {
    // ---- host operands (two scalars included): the executor's preallocation, then the reference kernel
    cp::ExecSpan stock_batch = batch;
    if (kd->swap_for_stock) std::swap(stock_batch.values[0], stock_batch.values[1]);
    ARROW_RETURN_NOT_OK(RunStockPrepared(kd->fn, kd->stock_exec, std::nullopt, 0, TwinValidity::kIntersection, ctx, stock_batch, out));
    if (out_arr->null_count < 0) {   // (this twin reports an exact count)
      out_arr->null_count = batch.length - arrow::internal::CountSetBits(out_arr->buffers[0]->data(), 0, batch.length);
    }
    return Status::OK();
  }
  if (any_host) {
    return Status::NotImplemented("arrow_amd: ", name, " of ", batch[0].type()->ToString(), " with one host and one device-resident array: "
                                  "both arrays of a device call live on the device");
  }
  const int64_t n = batch.length;
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  out_arr->buffers.assign(2, nullptr);
  out_arr->length = n;
  out_arr->offset = 0;
  const cp::ExecValue* scalar = !batch[0].is_array() ? &batch[0] : (!batch[1].is_array() ? &batch[1] : nullptr);
  if (scalar != nullptr && !scalar->scalar->is_valid) {   // every slot is null: nothing to compare
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[0], ZeroedDevice(BitmapBytes(n), st));
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], ZeroedDevice(BitmapBytes(n), st));
    out_arr->null_count = n;
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    CountGpu(kd->fn);
    return Status::OK();
  }
  ArxBinarySpan spans[2] = {};
  const ArxBinarySpan* side[2] = {nullptr, nullptr};
  int offset_width = 4;
  int64_t hint = 0;
  for (int i = 0; i < 2; ++i) {
    if (!batch[i].is_array()) continue;
    ARROW_RETURN_NOT_OK(DeviceBinarySpan(batch[i].array, &spans[i]));
    side[i] = &spans[i];
    offset_width = BinaryOffsetWidth(batch[i].array.type->id());
    hint += batch[i].array.buffers[2].size;
  }
  std::shared_ptr<Buffer> literal;
  int64_t m = 0;
  if (scalar != nullptr) {
    const std::string_view bytes = static_cast<const arrow::BaseBinaryScalar&>(*scalar->scalar).view();
    m = static_cast<int64_t>(bytes.size());
    ARROW_ASSIGN_OR_RAISE(literal, AllocDevice(std::max<int64_t>(m, 8)));
    if (m > 0) {
      HIP_RETURN_NOT_OK(hipMemcpyAsync(reinterpret_cast<void*>(literal->mutable_address()), bytes.data(), static_cast<size_t>(m),
                                       hipMemcpyHostToDevice, st));
    }
  }
  ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice(BitmapBytes(n)));
  ARROW_RETURN_NOT_OK(FromArx(arx_compare_binary(kd->op, side[0], side[1], offset_width,
                                                 literal != nullptr ? reinterpret_cast<const void*>(literal->address()) : nullptr, m, hint,
                                                 ARX_COMPARE_PATH_AUTO, reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address()), st)));
  // the validity: none when nothing can be null, a copy of the one bitmap that can hold nulls, the AND of two
  const ArxBinarySpan* with_nulls[2];
  int nv = 0;
  for (int i = 0; i < 2; ++i) {
    if (side[i] != nullptr && side[i]->validity != nullptr && side[i]->null_count != 0) with_nulls[nv++] = side[i];
  }
  out_arr->null_count = 0;
  if (nv == 1) {
    ARROW_RETURN_NOT_OK(CopyInputValidity(*with_nulls[0], n, st, out_arr));
  } else if (nv == 2) {
    ARROW_ASSIGN_OR_RAISE(auto valid, AllocDevice(BitmapBytes(n)));
    ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_and(with_nulls[0]->validity, with_nulls[0]->offset, with_nulls[1]->validity, with_nulls[1]->offset, n,
                                               reinterpret_cast<void*>(valid->mutable_address()), st)));
    ARROW_ASSIGN_OR_RAISE(out_arr->null_count, DeviceNullCount(*valid, n, st));
    if (out_arr->null_count != 0) out_arr->buffers[0] = valid;
  }
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (the literal and this thread's scratch may be released after return)
  CountGpu(kd->fn);
  return Status::OK();
}

// the added kernels: one per (function, type), appended after the reference's (dispatch takes the last match); the
// reference's own kernels stay behind the device guard (plugin/device_guard.inc)
Status RegisterStringCompare(cp::FunctionRegistry* reg) {
  const std::vector<ValueType> types = {arrow::utf8(), arrow::binary(), arrow::large_utf8(), arrow::large_binary()};
  // every twin first, while DispatchExact still finds the reference's kernels, then the additions
  std::vector<std::pair<cp::ScalarFunction*, cp::ScalarKernel>> twins;
  for (int op = ARX_CMP_EQUAL; op <= ARX_CMP_LESS_EQUAL; ++op) {
    const char* name = kStringCompareNames[op];
    const bool flipped = op == ARX_CMP_LESS || op == ARX_CMP_LESS_EQUAL;
    const char* source_name = op == ARX_CMP_LESS ? "greater" : op == ARX_CMP_LESS_EQUAL ? "greater_equal" : name;
    ARROW_ASSIGN_OR_RAISE(auto fn, reg->GetFunction(name));
    ARROW_ASSIGN_OR_RAISE(auto source, reg->GetFunction(source_name));
    if (fn->kind() != cp::Function::SCALAR || source->kind() != cp::Function::SCALAR) return Status::Invalid(name, " is not a scalar function");
    for (const ValueType& vt : types) {
      ARROW_ASSIGN_OR_RAISE(const cp::Kernel* k0, source->DispatchExact({vt.probe, vt.probe}));
      cp::ScalarKernel twin = *static_cast<const cp::ScalarKernel*>(k0);
      auto data = std::make_shared<StringCompareKernelData>();
      data->op = op;
      data->swap_for_stock = flipped;
      ARROW_RETURN_NOT_OK(InstallTwin(name, vt, &twin, !twin.init, std::move(data), kFnCompareString, nullptr, StringCompareExec,
                                      cp::KernelSignature::Make({vt.match, vt.match}, twin.signature->out_type())));
      twin.null_handling = cp::NullHandling::COMPUTED_NO_PREALLOCATE;
      twin.mem_allocation = cp::MemAllocation::NO_PREALLOCATE;
      twins.emplace_back(static_cast<cp::ScalarFunction*>(fn.get()), std::move(twin));
    }
  }
  for (auto& [fn, twin] : twins) ARROW_RETURN_NOT_OK(fn->AddKernel(std::move(twin)));
  return Status::OK();
}

// negate, abs (+ _checked), sign, floor, ceil, trunc, round, round_to_multiple on device-resident arrays
// (csrc/unary_arith.hip).
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- one-operand arithmetic and rounding
// The reference has one kernel per function and numeric type (scalar_arithmetic.cc, scalar_round.cc: INTERSECTION /
// PREALLOCATE); every one of the table in DESIGN.md 4.25 gets a twin.  A device-resident array runs arx_unary_numeric /
// arx_round_numeric into an HBM buffer, copies the input's bitmap (no bitmap when the input has no nulls), waits for the
// stream once and builds the Status from the error word; a host batch or a scalar runs the reference's exec behind the
// executor's preallocation contract (RunStockPrepared).  The reference's decimal, duration, half-float and null-type
// kernels of these functions, and all of round_binary, stay the reference's behind the device guard.
// round / round_to_multiple have an init: TwinInit runs the reference's first (its checks of the options — a null
// multiple, one that is not positive, one the column's type cannot hold — stay its own and come first), then keeps the
// options for the device call, which casts the multiple to the column's type the way that init did.
struct UnaryFunction {
  const char* name;
  int op;        // ARX_UNARY_*, or -1 - ARX_ROUND_* for the two rounding functions
  bool checked;
};
const UnaryFunction kUnaryFunctions[] = {
    {"negate", ARX_UNARY_NEGATE, false}, {"negate_checked", ARX_UNARY_NEGATE, true}, {"abs", ARX_UNARY_ABS, false},
    {"abs_checked", ARX_UNARY_ABS, true}, {"sign", ARX_UNARY_SIGN, false}, {"floor", ARX_UNARY_FLOOR, false},
    {"ceil", ARX_UNARY_CEIL, false}, {"trunc", ARX_UNARY_TRUNC, false}, {"round", -1 - ARX_ROUND_DIGITS, false},
    {"round_to_multiple", -1 - ARX_ROUND_MULTIPLE, false}};

struct UnaryKernelData : public TwinData {
  const UnaryFunction* function = nullptr;
};

int UnaryNumericTypeId(Type::type id) {
  switch (id) {
    case Type::INT8: return ARX_NUM_INT8;
    case Type::UINT8: return ARX_NUM_UINT8;
    case Type::INT16: return ARX_NUM_INT16;
    case Type::UINT16: return ARX_NUM_UINT16;
    case Type::INT32: return ARX_NUM_INT32;
    case Type::UINT32: return ARX_NUM_UINT32;
    case Type::INT64: return ARX_NUM_INT64;
    case Type::UINT64: return ARX_NUM_UINT64;
    case Type::FLOAT: return ARX_NUM_FLOAT32;
    case Type::DOUBLE: return ARX_NUM_FLOAT64;
    default: return -1;
  }
}

// RoundMode (api_scalar.h) -> ARX_ROUND_*: the same order, checked here rather than assumed
int UnaryRoundMode(cp::RoundMode mode) {
  switch (mode) {
    case cp::RoundMode::DOWN: return ARX_ROUND_DOWN;
    case cp::RoundMode::UP: return ARX_ROUND_UP;
    case cp::RoundMode::TOWARDS_ZERO: return ARX_ROUND_TOWARDS_ZERO;
    case cp::RoundMode::TOWARDS_INFINITY: return ARX_ROUND_TOWARDS_INFINITY;
    case cp::RoundMode::HALF_DOWN: return ARX_ROUND_HALF_DOWN;
    case cp::RoundMode::HALF_UP: return ARX_ROUND_HALF_UP;
    case cp::RoundMode::HALF_TOWARDS_ZERO: return ARX_ROUND_HALF_TOWARDS_ZERO;
    case cp::RoundMode::HALF_TOWARDS_INFINITY: return ARX_ROUND_HALF_TOWARDS_INFINITY;
    case cp::RoundMode::HALF_TO_EVEN: return ARX_ROUND_HALF_TO_EVEN;
    case cp::RoundMode::HALF_TO_ODD: return ARX_ROUND_HALF_TO_ODD;
  }
  return -1;
}

// The input's validity at offset 0 into out_arr->buffers[0] (none when it has no nulls) and its null count.
Status CopyNumericInputValidity(const ArxSpan& vs, int64_t n, hipStream_t st, ArrayData* out_arr) {
  out_arr->null_count = 0;
  if (vs.validity == nullptr || vs.null_count == 0 || n == 0) return Status::OK();
  ARROW_ASSIGN_OR_RAISE(auto valid, AllocDevice(BitmapBytes(n)));
  ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy(vs.validity, vs.offset, n, reinterpret_cast<void*>(valid->mutable_address()), st)));
  if (vs.null_count > 0) {
    out_arr->null_count = vs.null_count;
  } else {
    ARROW_ASSIGN_OR_RAISE(out_arr->null_count, DeviceNullCount(*valid, n, st));
  }
  if (out_arr->null_count != 0) out_arr->buffers[0] = valid;
  return Status::OK();
}

// the device half of both execs: `launch` (span, out, errors, stream) starts the kernel, `status` (errors, stream) waits
// for the stream and turns the error word into the Status
template <class Launch, class Finish>
Status UnaryOnDevice(Fn fn, const ArraySpan& rows, int out_width, Launch&& launch, Finish&& finish, cp::ExecResult* out) {
  const int64_t n = rows.length;
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  ArxSpan vs{};
  ARROW_RETURN_NOT_OK(DeviceSpan(rows, &vs));
  if (vs.null_count == 0) vs.validity = nullptr;
  ArrayData* out_arr = out->array_data().get();
  out_arr->buffers.assign(2, nullptr);
  ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice(std::max<int64_t>(n * out_width, 8)));
  void* f = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kFlag, 64, &f));
  HIP_RETURN_NOT_OK(hipMemsetAsync(f, 0, 8, st));
  uint64_t* d_errors = static_cast<uint64_t*>(f);
  ARROW_RETURN_NOT_OK(FromArx(launch(&vs, reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address()), d_errors, st)));
  ARROW_RETURN_NOT_OK(CopyNumericInputValidity(vs, n, st, out_arr));
  ARROW_RETURN_NOT_OK(finish(&vs, d_errors, st));   // (synchronizes: this thread's scratch may be released after return)
  CountGpu(fn);
  return Status::OK();
}

Status UnaryArithExecNP(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  const auto* kd = TwinDataOf<UnaryKernelData>(ctx->kernel());
  if (kd == nullptr || kd->function == nullptr) return TwinWithoutData();
  const UnaryFunction& f = *kd->function;
  const int out_width = out->type()->byte_width();
  if (!batch[0].is_array() || !SpanTouchesRocm(batch[0].array)) {
    return RunStockPrepared(kd->fn, kd->stock_exec, std::nullopt, out_width, TwinValidity::kIntersection, ctx, batch, out);
  }
  const ArraySpan& rows = batch[0].array;
  const int num = UnaryNumericTypeId(rows.type->id());
  if (num < 0) return Status::Invalid("arrow_amd: ", f.name, " twin matched ", rows.type->ToString());
  return UnaryOnDevice(
      kd->fn, rows, out_width,
      [&](const ArxSpan* vs, void* d_out, uint64_t* d_errors, hipStream_t st) {
        return arx_unary_numeric(f.op, f.checked ? 1 : 0, num, vs, d_out, d_errors, st);
      },
      [&](const ArxSpan*, const uint64_t* d_errors, hipStream_t st) -> Status {
        uint64_t last = 0;
        if (f.checked) HIP_RETURN_NOT_OK(hipMemcpyAsync(&last, d_errors, 8, hipMemcpyDeviceToHost, st));
        HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
        return last != 0 ? Status::Invalid("overflow") : Status::OK();   // NegateChecked / AbsoluteValueChecked::Call
      },
      out);
}

template <class Options>
Status RoundExecNP(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  const auto* kd = TwinDataOf<UnaryKernelData>(ctx->kernel());
  if (kd == nullptr || kd->function == nullptr || !kd->stock_init) return TwinWithoutData();
  const UnaryFunction& f = *kd->function;
  auto* state = static_cast<ShimState<Options>*>(ctx->state());
  if (state == nullptr) return Status::Invalid("arrow_amd: ", f.name, " ran without its state");
  const int out_width = out->type()->byte_width();
  if (!batch[0].is_array() || !SpanTouchesRocm(batch[0].array)) {
    return RunStockPrepared(kd->fn, kd->stock_exec, std::optional<cp::KernelState*>(state->stock.get()), out_width,
                            TwinValidity::kIntersection, ctx, batch, out);
  }
  const ArraySpan& rows = batch[0].array;
  const int num = UnaryNumericTypeId(rows.type->id());
  if (num < 0) return Status::Invalid("arrow_amd: ", f.name, " twin matched ", rows.type->ToString());
  const int kind = -1 - f.op;
  const int mode = UnaryRoundMode(state->options.round_mode);
  int64_t ndigits = 0;
  uint64_t multiple_bytes = 0;
  const void* multiple = nullptr;
  if constexpr (std::is_same<Options, cp::RoundOptions>::value) {
    ndigits = state->options.ndigits;
  } else {
    // the reference's init has accepted this multiple for this column type: the same safe cast cannot fail here
    if (state->options.multiple == nullptr || !state->options.multiple->is_valid) {
      return Status::Invalid("Rounding multiple must be non-null and valid");
    }
    ARROW_ASSIGN_OR_RAISE(arrow::Datum cast, cp::Cast(arrow::Datum(state->options.multiple), rows.type->GetSharedPtr(), cp::CastOptions::Safe(),
                                                      ctx->exec_context()));
    if (!cast.is_scalar() || FixedWidthScalarBytes(*cast.scalar(), out_width, &multiple_bytes) != out_width) {
      return Status::Invalid("arrow_amd: ", f.name, ": the multiple did not cast to ", rows.type->ToString());
    }
    multiple = &multiple_bytes;
  }
  return UnaryOnDevice(
      kd->fn, rows, out_width,
      [&](const ArxSpan* vs, void* d_out, uint64_t* d_errors, hipStream_t st) {
        return arx_round_numeric(kind, mode, num, vs, ndigits, multiple, d_out, d_errors, st);
      },
      [&](const ArxSpan* vs, const uint64_t* d_errors, hipStream_t st) -> Status {
        return FromArx(arx_round_status(kind, mode, num, vs, ndigits, multiple, d_errors, st));
      },
      out);
}

// one twin per function and numeric type of the reference's lists, appended after the reference's kernels (dispatch takes
// the last match); the reference's own kernels stay behind the device guard (plugin/device_guard.inc)
Status RegisterUnaryArith(cp::FunctionRegistry* reg) {
  const std::vector<std::shared_ptr<arrow::DataType>> numeric = {arrow::int8(),  arrow::uint8(),  arrow::int16(),   arrow::uint16(), arrow::int32(),
                                                                  arrow::uint32(), arrow::int64(), arrow::uint64(), arrow::float32(), arrow::float64()};
  for (const UnaryFunction& f : kUnaryFunctions) {
    std::vector<ValueType> types;
    for (const auto& t : numeric) {
      const bool floating = arrow::is_floating(t->id());
      if (f.op >= ARX_UNARY_FLOOR && !floating) continue;                                            // floor, ceil, trunc: floats only
      if (f.op == ARX_UNARY_NEGATE && f.checked && arrow::is_unsigned_integer(t->id())) continue;   // no unsigned negate_checked
      types.emplace_back(t);
    }
    const UnaryFunction* row = &f;
    ARROW_RETURN_NOT_OK(AppendTwins(
        reg, f.name, types, [](const auto& t) { return std::vector<arrow::TypeHolder>{t}; },
        [=](const ValueType& vt, cp::ScalarKernel* twin) -> arrow::Result<bool> {
          auto data = std::make_shared<UnaryKernelData>();
          data->function = row;
          const bool rounds = row->op < 0;
          const Fn fn = rounds ? kFnRound : kFnUnaryArith;
          if (!rounds) {
            ARROW_RETURN_NOT_OK(InstallTwin(row->name, vt, twin, !twin->init, std::move(data), fn, nullptr, UnaryArithExecNP));
          } else if (-1 - row->op == ARX_ROUND_DIGITS) {
            ARROW_RETURN_NOT_OK(InstallTwin(row->name, vt, twin, static_cast<bool>(twin->init), std::move(data), fn, TwinInit<cp::RoundOptions>,
                                            RoundExecNP<cp::RoundOptions>));
          } else {
            ARROW_RETURN_NOT_OK(InstallTwin(row->name, vt, twin, static_cast<bool>(twin->init), std::move(data), fn,
                                            TwinInit<cp::RoundToMultipleOptions>, RoundExecNP<cp::RoundToMultipleOptions>));
          }
          return true;
        }));
  }
  return Status::OK();
}

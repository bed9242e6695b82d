// Element-wise shims: compare family, arithmetic (+checked), Kleene logic.
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- compare / arithmetic / divide on the numeric types
// One Op per (function, element type) describes a NO_PREALLOCATE kernel (ScalarBinaryNP below): NullHandling::
// COMPUTED_NO_PREALLOCATE + MemAllocation::NO_PREALLOCATE, because the ScalarExecutor's own preallocation and null
// propagation (exec.cc:846-861,1222-1281) run on the CPU and cannot touch device buffers.
//  * device-resident operands (arrays, or one scalar): the operation, the validity intersection and the null count all
//    run on the MI355X and the result stays in HBM (so compare -> filter chains never leave the device);
//  * host operands get exactly the buffers the ScalarExecutor would have preallocated and then go to Arrow's stock
//    kernel (these element-wise ops are PCIe-bound for host data).
// NUM = ARX_NUM_*: the library picks the device kernel for the type.  SLOT: one stock-kernel slot per (function, type).
// FN: the arrow_amd_plugin_calls counter the Op reports under.
StockKernel g_stock_compare[6 * 10];
StockKernel g_stock_arith[6 * 10];
StockKernel g_stock_divide[2 * 10];

// "greater" on int64 / double has a counter of its own (it predates the family; the benchmark's greater leg reads it),
// every other comparison reports under "compare"
template <typename CT, int CMP>
constexpr Fn kCompareFn = CMP == ARX_CMP_GREATER && (std::is_same<CT, int64_t>::value || std::is_same<CT, double>::value)
                              ? kFnGreater : kFnCompare;

template <typename CT, typename ScalarType, int NUM, int CMP, int SLOT, Fn FN = kCompareFn<CT, CMP>>
struct OpCompare {
  using T = CT;
  using ScalarT = ScalarType;
  static constexpr bool kBitmapOut = true;
  static constexpr bool kChecked = false;
  static constexpr Fn kFn = FN;
  // greater(double, double) on large HOST arrays is staged through HBM (StagedHostCompare) instead of going to the stock kernel
  static constexpr bool kStageHostArrays = CMP == ARX_CMP_GREATER && std::is_same<CT, double>::value;
  static StockKernel& stock() { return g_stock_compare[SLOT]; }
  static int run(const T* l, T ls, const T* r, T rs, int64_t n, void* o, hipStream_t st) {
    return arx_compare_numeric(CMP, NUM, l, &ls, r, &rs, n, static_cast<uint64_t*>(o), st);
  }
  static int aa(const T* l, const T* r, int64_t n, void* o, hipStream_t st) { return run(l, T(0), r, T(0), n, o, st); }
  static int as(const T* l, T r, int64_t n, void* o, hipStream_t st) { return run(l, T(0), nullptr, r, n, o, st); }
  static int sa(T l, const T* r, int64_t n, void* o, hipStream_t st) { return run(nullptr, l, r, T(0), n, o, st); }
};

// add / subtract / multiply and add_checked / subtract_checked / multiply_checked: what `+`, `-`, `*` on pyarrow /
// Acero expressions mean.  The checked integer forms read an overflow flag back after the kernel and fail with the
// reference's Status::Invalid("overflow").
template <typename CT, typename ScalarType, int NUM, int OP, bool CHECKED, int SLOT>
struct OpArith {
  using T = CT;
  using ScalarT = ScalarType;
  static constexpr bool kBitmapOut = false;
  static constexpr bool kChecked = CHECKED && std::is_integral<CT>::value;
  static constexpr Fn kFn = kFnAdd;
  static StockKernel& stock() { return g_stock_arith[SLOT]; }
  static int run(const T* l, T ls, const T* r, T rs, int64_t n, void* o, hipStream_t st) {
    return arx_arith_numeric(OP, 0, NUM, l, &ls, nullptr, 0, r, &rs, nullptr, 0, n, o, nullptr, st);
  }
  static int aa(const T* l, const T* r, int64_t n, void* o, hipStream_t st) { return run(l, T(0), r, T(0), n, o, st); }
  static int as(const T* l, T r, int64_t n, void* o, hipStream_t st) { return run(l, T(0), nullptr, r, n, o, st); }
  static int sa(T l, const T* r, int64_t n, void* o, hipStream_t st) { return run(nullptr, l, r, T(0), n, o, st); }
  static int checked(const T* l, T ls, const ArxSpan& lsp, const T* r, T rs, const ArxSpan& rsp, int64_t n, void* o,
                     unsigned int* flag, hipStream_t st) {
    return arx_arith_numeric(OP, 1, NUM, l, &ls, l ? lsp.validity : nullptr, lsp.offset, r, &rs, r ? rsp.validity : nullptr,
                             rsp.offset, n, o, flag, st);
  }
};

// The comparisons for the temporal types (timestamp, duration, time32 / time64 per unit; date32, date64): their values
// are int32 / int64 and compare as such (the reference registers the Int32 / Int64 bodies for them,
// scalar_compare.cc:400-431).  Timestamps: comparing a zoned with a zone-less column is an error in the reference
// (CompareTimestamps, scalar_compare.cc:299-313) — checked here for device operands, by the stock exec for host ones.
StockKernel g_stock_compare_temporal[6 * 14];

template <typename CT, typename ScalarType, int NUM, int CMP, int SLOT>
struct OpCompareTemporal : OpCompare<CT, ScalarType, NUM, CMP, SLOT, kFnCompare> {
  static StockKernel& stock() { return g_stock_compare_temporal[SLOT]; }
  static constexpr bool kTemporal = true;
  // less / less_equal are greater / greater_equal with the operands swapped in the reference (scalar_compare.cc:436-445):
  // its error text names the types in that order
  static constexpr bool kFlipped = CMP == ARX_CMP_LESS || CMP == ARX_CMP_LESS_EQUAL;
};
template <class Op, class = void>
struct IsTemporalOp : std::false_type {};
template <class Op>
struct IsTemporalOp<Op, std::void_t<decltype(Op::kTemporal)>> : std::true_type {};

// divide / divide_checked: Divide / DivideChecked, base_arithmetic_internal.h:366-424.  Both forms can fail ("divide by
// zero"; the checked one also "overflow" for min / -1 of a signed type): the kernel leaves the last failing row of each
// kind in two device words, the larger one names the Status (the reference overwrites it slot by slot).
template <typename CT, typename ScalarType, int NUM, bool CHECKED, int SLOT>
struct OpDivide {
  using T = CT;
  using ScalarT = ScalarType;
  static constexpr bool kBitmapOut = false;
  static constexpr bool kChecked = false;
  static constexpr bool kDivideChecked = CHECKED;
  static constexpr Fn kFn = kFnAdd;
  static StockKernel& stock() { return g_stock_divide[SLOT]; }
  static int aa(const T*, const T*, int64_t, void*, hipStream_t) { return ARX_NOT_IMPLEMENTED; }
  static int as(const T*, T, int64_t, void*, hipStream_t) { return ARX_NOT_IMPLEMENTED; }
  static int sa(T, const T*, int64_t, void*, hipStream_t) { return ARX_NOT_IMPLEMENTED; }
  static int divide(const T* l, T ls, const ArxSpan& lsp, const T* r, T rs, const ArxSpan& rsp, int64_t n, void* o,
                    uint64_t* errors, hipStream_t st) {
    return arx_divide_numeric(CHECKED ? 1 : 0, NUM, l, &ls, l ? lsp.validity : nullptr, lsp.offset, r, &rs,
                              r ? rsp.validity : nullptr, rsp.offset, n, o, errors, st);
  }
};
template <class Op, class = void>
struct IsDivideOp : std::false_type {};
template <class Op>
struct IsDivideOp<Op, std::void_t<decltype(Op::kDivideChecked)>> : std::true_type {};

template <class Op, class = void>
struct StagesHostArrays : std::false_type {};
template <class Op>
struct StagesHostArrays<Op, std::void_t<decltype(Op::kStageHostArrays)>> : std::bool_constant<Op::kStageHostArrays> {};

// The host half of an Op with kStageHostArrays: two host arrays of at least g_min_rows_streaming rows are copied to HBM,
// compared there and the bitmap copied back into the preallocated output (counted as a GPU call); scalars and small
// inputs go to Arrow's stock kernel.  Validity has been propagated by the caller.
template <class Op>
Status StagedHostCompare(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  using T = typename Op::T;
  if (!batch[0].is_array() || !batch[1].is_array() || !out->is_array_span() ||
      out->array_span()->offset != 0 || batch.length < g_min_rows_streaming.load() ||
      !IsHost(batch[0].array) || !IsHost(batch[1].array)) {
    CountStock(Op::kFn);
    return Op::stock().exec(ctx, batch, out);
  }
  const ArraySpan& l = batch[0].array;
  const ArraySpan& r = batch[1].array;
  const int64_t n = batch.length;
  const size_t bytes = static_cast<size_t>(n) * sizeof(T);
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  void *dl = nullptr, *dr = nullptr, *dout = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kValues, bytes, &dl));
  ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2, bytes, &dr));
  ARROW_RETURN_NOT_OK(t_scratch.Get(kOutData, static_cast<size_t>((n + 63) / 64) * 8, &dout));
  HIP_RETURN_NOT_OK(hipMemcpyAsync(dl, l.GetValues<T>(1), bytes, hipMemcpyHostToDevice, st));
  HIP_RETURN_NOT_OK(hipMemcpyAsync(dr, r.GetValues<T>(1), bytes, hipMemcpyHostToDevice, st));
  ARROW_RETURN_NOT_OK(FromArx(Op::aa(static_cast<const T*>(dl), static_cast<const T*>(dr), n, dout, st)));
  ArraySpan* o = out->array_span_mutable();
  HIP_RETURN_NOT_OK(hipMemcpyAsync(o->buffers[1].data, dout, static_cast<size_t>(arrow::bit_util::BytesForBits(n)),
                                   hipMemcpyDeviceToHost, st));
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  CountGpu(Op::kFn);
  return Status::OK();
}

template <class Op>
Status ScalarBinaryNP(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  using T = typename Op::T;
  const int64_t n = batch.length;
  ArrayData* out_arr = out->array_data().get();
  out_arr->buffers.resize(2);
  const bool dev0 = batch[0].is_array() && OnRocm(batch[0].array);
  const bool dev1 = batch[1].is_array() && OnRocm(batch[1].array);
  const int64_t data_bytes = Op::kBitmapOut ? ((n + 63) / 64) * 8 : n * static_cast<int64_t>(sizeof(T));
  if (dev0 || dev1) {
    bool null_scalar = false;
    for (int i = 0; i < 2; ++i) {
      if (batch[i].is_array() && !OnRocm(batch[i].array)) {
        return Status::NotImplemented("arrow_amd: ", kFnNames[Op::kFn], " on device-resident arrays needs device "
                                      "arrays or scalars on both sides");
      }
      null_scalar = null_scalar || (batch[i].is_scalar() && !batch[i].scalar->is_valid);
    }
    if (null_scalar) {
      // a null scalar operand: every slot of the result is null and no slot is visited (ScalarBinaryNotNull /
      // PropagateNulls, codegen_internal.h, exec.cc) — zeroed values under an all-clear validity bitmap, in HBM
      hipStream_t st;
      ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
      ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice(std::max<int64_t>(data_bytes, 8)));
      ARROW_ASSIGN_OR_RAISE(out_arr->buffers[0], AllocDevice(BitmapBytes(n)));
      HIP_RETURN_NOT_OK(hipMemsetAsync(reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address()), 0,
                                       static_cast<size_t>(std::max<int64_t>(data_bytes, 8)), st));
      HIP_RETURN_NOT_OK(hipMemsetAsync(reinterpret_cast<void*>(out_arr->buffers[0]->mutable_address()), 0,
                                       static_cast<size_t>(BitmapBytes(n)), st));
      HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
      out_arr->null_count = n;
      CountGpu(Op::kFn);
      return Status::OK();
    }
    if constexpr (IsTemporalOp<Op>::value) {
      const arrow::DataType* t0 = batch[Op::kFlipped ? 1 : 0].type();
      const arrow::DataType* t1 = batch[Op::kFlipped ? 0 : 1].type();
      if (t0->id() == Type::TIMESTAMP && t1->id() == Type::TIMESTAMP) {
        const bool z0 = !static_cast<const arrow::TimestampType&>(*t0).timezone().empty();
        const bool z1 = !static_cast<const arrow::TimestampType&>(*t1).timezone().empty();
        if (z0 != z1) {
          return Status::Invalid("Cannot compare timestamp with timezone to timestamp without timezone, got: ",
                                 t0->ToString(), " and ", t1->ToString());
        }
      }
    }
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice(data_bytes));
    void* dout = reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address());
    ArxSpan sp[2] = {};
    const T* ptr[2] = {nullptr, nullptr};
    T sc[2] = {T(0), T(0)};
    for (int i = 0; i < 2; ++i) {
      if (batch[i].is_array()) {
        ARROW_RETURN_NOT_OK(DeviceSpan(batch[i].array, &sp[i]));
        ptr[i] = static_cast<const T*>(sp[i].data) + sp[i].offset;
      } else {
        sc[i] = static_cast<const typename Op::ScalarT&>(*batch[i].scalar).value;
      }
    }
    int rc;
    unsigned int* d_flag = nullptr;
    uint64_t* d_errors = nullptr;
    if constexpr (IsDivideOp<Op>::value) {
      void* f = nullptr;
      ARROW_RETURN_NOT_OK(t_scratch.Get(kFlag, 64, &f));
      HIP_RETURN_NOT_OK(hipMemsetAsync(f, 0, 16, st));
      d_errors = static_cast<uint64_t*>(f);
      rc = Op::divide(ptr[0], sc[0], sp[0], ptr[1], sc[1], sp[1], n, dout, d_errors, st);
    } else if constexpr (Op::kChecked) {
      void* f = nullptr;
      ARROW_RETURN_NOT_OK(t_scratch.Get(kFlag, 64, &f));
      HIP_RETURN_NOT_OK(hipMemsetAsync(f, 0, 4, st));
      d_flag = static_cast<unsigned int*>(f);
      rc = Op::checked(ptr[0], sc[0], sp[0], ptr[1], sc[1], sp[1], n, dout, d_flag, st);
    } else {
      if (ptr[0] && ptr[1]) rc = Op::aa(ptr[0], ptr[1], n, dout, st);
      else if (ptr[0]) rc = Op::as(ptr[0], sc[1], n, dout, st);
      else rc = Op::sa(sc[0], ptr[1], n, dout, st);
    }
    ARROW_RETURN_NOT_OK(FromArx(rc));
    const ArxSpan* with_nulls[2];
    int nv = 0;
    for (int i = 0; i < 2; ++i) {
      if (ptr[i] && sp[i].validity != nullptr) with_nulls[nv++] = &sp[i];
    }
    out_arr->buffers[0] = nullptr;
    out_arr->null_count = 0;
    if (nv > 0 && n > 0) {
      ARROW_ASSIGN_OR_RAISE(out_arr->buffers[0], AllocDevice(((n + 63) / 64) * 8));
      void* dv = reinterpret_cast<void*>(out_arr->buffers[0]->mutable_address());
      if (nv == 1) {
        ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy(with_nulls[0]->validity, with_nulls[0]->offset, n, dv, st)));
      } else {
        ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_and(with_nulls[0]->validity, with_nulls[0]->offset,
                                                   with_nulls[1]->validity, with_nulls[1]->offset, n, dv, st)));
      }
      ARROW_ASSIGN_OR_RAISE(out_arr->null_count, DeviceNullCount(*out_arr->buffers[0], n, st));
    }
    unsigned int flag = 0;
    uint64_t errors[2] = {0, 0};
    if (d_flag != nullptr) HIP_RETURN_NOT_OK(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    if (d_errors != nullptr) HIP_RETURN_NOT_OK(hipMemcpyAsync(errors, d_errors, 16, hipMemcpyDeviceToHost, st));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    if (flag != 0) return Status::Invalid("overflow");  // AddChecked::Call, base_arithmetic_internal.h:77
    if (errors[1] > errors[0]) return Status::Invalid("divide by zero");   // Divide::Call :377-380 (the last failing slot wins)
    if (errors[0] != 0) return Status::Invalid("overflow");                // DivideChecked::Call :405-410
    CountGpu(Op::kFn);
    return Status::OK();
  }

  // ---- host operands: ScalarExecutor::PrepareOutput + PropagateNulls, then Arrow's stock kernel (or the Op's staging)
  const int width = Op::kBitmapOut ? 0 : static_cast<int>(sizeof(T));
  if constexpr (StagesHostArrays<Op>::value) {
    PreparedOutput p;
    ARROW_RETURN_NOT_OK(p.Prepare(ctx, batch, out_arr->type.get(), width, TwinValidity::kIntersection));
    ARROW_RETURN_NOT_OK(StagedHostCompare<Op>(ctx, batch, &p.tmp));
    p.MoveInto(out_arr);
    return Status::OK();
  } else {
    return RunStockPrepared(Op::kFn, Op::stock().exec, std::nullopt, width, TwinValidity::kIntersection, ctx, batch, out);
  }
}

// vt.match: the matcher the added kernel is registered under when the type is parametric (timestamp(unit, any zone) ...);
// the stock kernel is found with the concrete probe type either way.
template <class Op>
Status RegisterScalarBinaryNP(cp::FunctionRegistry* reg, const char* name, const ValueType& vt) {
  return AppendTwins(reg, name, {vt}, [](const auto& t) { return std::vector<arrow::TypeHolder>{t, t}; },
                     [](const ValueType& v, cp::ScalarKernel* twin) -> arrow::Result<bool> {
                       Op::stock().exec = twin->exec;
                       Op::stock().init = twin->init;
                       twin->signature = cp::KernelSignature::Make({v.match, v.match}, twin->signature->out_type());
                       twin->exec = ScalarBinaryNP<Op>;
                       return true;
                     });
}

// ---------------------------------------------------------------- and_kleene / or_kleene / invert
// What Acero filter expressions like (a > 1) & (b > 2) evaluate to.  Same NO_PREALLOCATE twin:
// device-resident boolean arrays run arx_boolean_kleene / arx_boolean_invert and stay in HBM; host
// operands get the buffers the executor would have preallocated (data + validity bitmaps) and go to
// Arrow's stock kernel.
StockKernel g_stock_and_kleene, g_stock_or_kleene, g_stock_invert;

template <int OP>
Status KleeneExecNP(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  StockKernel& stock = OP == ARX_AND_KLEENE ? g_stock_and_kleene : g_stock_or_kleene;
  const int64_t n = batch.length;
  ArrayData* out_arr = out->array_data().get();
  out_arr->buffers.resize(2);
  const bool dev0 = batch[0].is_array() && OnRocm(batch[0].array);
  const bool dev1 = batch[1].is_array() && OnRocm(batch[1].array);
  if (dev0 || dev1) {
    for (int i = 0; i < 2; ++i) {
      if (batch[i].is_array() && !OnRocm(batch[i].array)) {
        return Status::NotImplemented("arrow_amd: and_kleene / or_kleene on device-resident arrays needs device "
                                      "arrays or scalars on both sides");
      }
    }
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    const int64_t bytes = ((n + 63) / 64) * 8;
    // a scalar operand (true / false / null) is broadcast into scratch bitmaps and takes the array path: Kleene logic
    // has no shortcut that holds for all three (scalar_boolean.cc KleeneAndOp / KleeneOrOp visit it per slot too)
    ArxSpan sp[2] = {};
    for (int i = 0; i < 2; ++i) {
      if (batch[i].is_array()) {
        ARROW_RETURN_NOT_OK(DeviceSpan(batch[i].array, &sp[i]));
        continue;
      }
      const arrow::Scalar& sc = *batch[i].scalar;
      const bool value = sc.is_valid && static_cast<const arrow::BooleanScalar&>(sc).value;
      void *bits = nullptr, *valid = nullptr;
      ARROW_RETURN_NOT_OK(t_scratch.Get(i == 0 ? kValues : kArg2, static_cast<size_t>(bytes) + 16, &bits));
      HIP_RETURN_NOT_OK(hipMemsetAsync(bits, value ? 0xFF : 0, static_cast<size_t>(bytes) + 16, st));
      if (!sc.is_valid) {
        ARROW_RETURN_NOT_OK(t_scratch.Get(i == 0 ? kValidity : kArg2Validity, static_cast<size_t>(bytes) + 16, &valid));
        HIP_RETURN_NOT_OK(hipMemsetAsync(valid, 0, static_cast<size_t>(bytes) + 16, st));
      }
      sp[i] = ArxSpan{valid, bits, 0, n, sc.is_valid ? 0 : n};
    }
    const ArxSpan &l = sp[0], &r = sp[1];
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice(bytes));
    out_arr->buffers[0] = nullptr;
    void* dvalid = nullptr;
    const bool nulls = l.validity != nullptr || r.validity != nullptr;
    if (nulls) {
      ARROW_ASSIGN_OR_RAISE(out_arr->buffers[0], AllocDevice(bytes));
      dvalid = reinterpret_cast<void*>(out_arr->buffers[0]->mutable_address());
    }
    ARROW_RETURN_NOT_OK(FromArx(arx_boolean_kleene(OP, &l, &r, reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address()),
                                                   dvalid, st)));
    out_arr->null_count = 0;
    if (nulls && n > 0) {
      ARROW_ASSIGN_OR_RAISE(out_arr->null_count, DeviceNullCount(*out_arr->buffers[0], n, st));
    }
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    CountGpu(kFnBoolean);
    return Status::OK();
  }
  // host operands: NullHandling::COMPUTED_PREALLOCATE + MemAllocation::PREALLOCATE of the stock kernel
  int64_t null_count = 0;
  ARROW_RETURN_NOT_OK(RunStockPrepared(kFnBoolean, stock.exec, std::nullopt, 0, TwinValidity::kAllocate, ctx, batch, out, &null_count));
  out_arr->null_count = null_count;   // (as the reference's exec counted it)
  return Status::OK();
}

Status InvertExecNP(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  const int64_t n = batch.length;
  ArrayData* out_arr = out->array_data().get();
  out_arr->buffers.resize(2);
  if (batch[0].is_array() && OnRocm(batch[0].array)) {
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    ArxSpan a{};
    ARROW_RETURN_NOT_OK(DeviceSpan(batch[0].array, &a));
    const int64_t bytes = ((n + 63) / 64) * 8;
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice(bytes));
    ARROW_RETURN_NOT_OK(FromArx(arx_boolean_invert(a.data, a.offset, n,
                                                   reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address()), st)));
    out_arr->buffers[0] = nullptr;
    out_arr->null_count = 0;
    if (a.validity != nullptr && n > 0) {
      ARROW_ASSIGN_OR_RAISE(out_arr->buffers[0], AllocDevice(bytes));
      ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy(a.validity, a.offset, n,
                                                  reinterpret_cast<void*>(out_arr->buffers[0]->mutable_address()), st)));
      ARROW_ASSIGN_OR_RAISE(out_arr->null_count, DeviceNullCount(*out_arr->buffers[0], n, st));
    }
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    CountGpu(kFnBoolean);
    return Status::OK();
  }
  // host operand: NullHandling::INTERSECTION + PREALLOCATE
  return RunStockPrepared(kFnBoolean, g_stock_invert.exec, std::nullopt, 0, TwinValidity::kIntersection, ctx, batch, out);
}

Status RegisterBooleanNP(cp::FunctionRegistry* reg, const char* name, int arity, cp::ArrayKernelExec exec,
                         StockKernel* stock) {
  return AppendTwins(reg, name, {arrow::boolean()},
                     [arity](const auto& t) { return std::vector<arrow::TypeHolder>(arity, t); },
                     [=](const ValueType&, cp::ScalarKernel* twin) -> arrow::Result<bool> {
                       stock->exec = twin->exec;
                       stock->init = twin->init;
                       twin->exec = exec;   // (the reference's signature stays)
                       return true;
                     });
}

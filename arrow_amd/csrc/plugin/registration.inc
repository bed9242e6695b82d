// Registration of every shim on the live FunctionRegistry / exec-factory registry.
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- registration
std::vector<ValueType> FilterValueTypes() {
  return {arrow::boolean(), arrow::int8(), arrow::uint8(), arrow::int16(), arrow::uint16(), arrow::int32(), arrow::uint32(),
          arrow::int64(), arrow::uint64(), arrow::float16(), arrow::float32(), arrow::float64(), arrow::date32(),
          arrow::date64(), arrow::month_interval(), arrow::day_time_interval(), arrow::month_day_nano_interval(),
          {arrow::time32(arrow::TimeUnit::SECOND), Type::TIME32},
          {arrow::time64(arrow::TimeUnit::NANO), Type::TIME64},
          {arrow::timestamp(arrow::TimeUnit::NANO), Type::TIMESTAMP},
          {arrow::duration(arrow::TimeUnit::NANO), Type::DURATION},
          {arrow::decimal128(38, 9), Type::DECIMAL128},
          {arrow::decimal256(60, 9), Type::DECIMAL256},
          {arrow::fixed_size_binary(16), Type::FIXED_SIZE_BINARY}};
}

Status RegisterVector(cp::FunctionRegistry* reg, const std::string& name,
                      const std::vector<ValueType>& first_types,
                      const std::vector<cp::InputType>& second, cp::KernelInit init,
                      cp::ArrayKernelExec exec, StockKernel* stock,
                      cp::VectorKernel::ChunkedExec chunked = nullptr) {
  ARROW_ASSIGN_OR_RAISE(auto fn, reg->GetFunction(name));
  if (fn->kind() != cp::Function::VECTOR) return Status::Invalid(name, " is not a vector function");
  auto* vfn = static_cast<cp::VectorFunction*>(fn.get());
  for (const auto& vt : first_types) {
    std::vector<arrow::TypeHolder> probe{vt.probe};
    std::vector<cp::InputType> in{vt.match};
    if (!second.empty()) {
      // probe with a concrete second argument type
      probe.push_back(name == "array_filter" ? arrow::boolean() : arrow::int32());
    }
    ARROW_ASSIGN_OR_RAISE(const cp::Kernel* k0, vfn->DispatchExact(probe));
    cp::VectorKernel copy = *static_cast<const cp::VectorKernel*>(k0);
    if (stock->exec == nullptr) {
      stock->exec = copy.exec;
      stock->init = copy.init;
      stock->exec_chunked = copy.exec_chunked;
    } else if (stock->exec != copy.exec) {
      continue;  // a different stock kernel handles this type: leave it alone
    }
    for (const auto& s : second) in.push_back(s);
    copy.signature = cp::KernelSignature::Make(in, copy.signature->out_type());
    copy.init = init;
    copy.exec = exec;
    if (name == "array_sort_indices") {
      copy.mem_allocation = cp::MemAllocation::NO_PREALLOCATE;
      if (copy.exec_chunked != nullptr) copy.exec_chunked = chunked;
    }
    ARROW_RETURN_NOT_OK(vfn->AddKernel(std::move(copy)));
  }
  return Status::OK();
}

Status RegisterAll() {
  ARROW_RETURN_NOT_OK(cp::Initialize());
  const int ndev = arx_device_count();
  // ARROW_AMD_PLUGIN_DRY_RUN=1: register without a device so the registration logic itself can be
  // exercised on a GPU-less box (tests/test_plugin_registration.py); any call large enough to be
  // routed to the HIP kernels then fails loudly with a HIP error — nothing computes on the CPU here.
  const char* dry = std::getenv("ARROW_AMD_PLUGIN_DRY_RUN");
  if (ndev < 1 && !(dry != nullptr && dry[0] == '1')) {
    return Status::Invalid("arrow_amd: no HIP device visible (", arx_last_error(),
                           "); nothing registered, Arrow keeps its stock kernels");
  }
  // arrays can now be imported onto the MI355X through the C Device Data interface
  {
    const Status st = arrow::RegisterDeviceMapper(arrow::DeviceAllocationType::kROCM, RocmMemoryManagerFor);
    if (!st.ok() && !st.IsKeyError()) return st;  // KeyError: somebody registered kROCM before us
  }
  cp::FunctionRegistry* reg = cp::GetFunctionRegistry();
  ARROW_ASSIGN_OR_RAISE(const std::vector<int> stock_kernel_counts, CountStockKernels(reg));   // (plugin/device_guard.inc)
  SnapshotStockAggregateKernels(reg);   // (plugin/acero_override.inc: what the aggregate guard must keep away from device values)
  // run_end_encoded<*, boolean> filters: the same exec (the reference's PrimitiveFilterExec takes both filter layouts,
  // vector_selection_filter_internal.cc:1090,1116-1124); host arrays go on to the stock kernel, device arrays expand
  // the runs on the device first.  (Registered BEFORE the plain-mask kernels: RegisterVector finds the stock exec by
  // dispatching on a plain boolean mask, which must still reach the reference's kernel at that point.)
  ARROW_RETURN_NOT_OK(RegisterVector(reg, "array_filter", FilterValueTypes(),
                                     {cp::InputType(cp::match::RunEndEncoded(Type::BOOL))}, FilterInit, FilterExec,
                                     &g_stock_filter));
  ARROW_RETURN_NOT_OK(RegisterVector(reg, "array_filter", FilterValueTypes(), {cp::InputType(arrow::boolean())},
                                     FilterInit, FilterExec, &g_stock_filter));
  ARROW_RETURN_NOT_OK(RegisterVector(reg, "array_take", FilterValueTypes(),
                                     {cp::InputType(cp::match::Integer())}, TakeInit, TakeExec,
                                     &g_stock_take));
  ARROW_RETURN_NOT_OK(RegisterVector(reg, "array_filter", {arrow::utf8(), arrow::binary()},
                                     {cp::InputType(arrow::boolean())}, BinaryFilterInit, BinaryFilterExec,
                                     &g_stock_filter_bin));
  ARROW_RETURN_NOT_OK(RegisterVector(reg, "array_take", {arrow::utf8(), arrow::binary()},
                                     {cp::InputType(cp::match::Integer())}, BinaryTakeInit, BinaryTakeExec,
                                     &g_stock_take_bin));
  // round 4: large_utf8 / large_binary (int64 offsets) through the same kernels (arx_large_binary_take_*); the reference
  // runs all four types through one VarBinary implementation, so the stock kernel recorded above serves their host batches
  ARROW_RETURN_NOT_OK(RegisterVector(reg, "array_filter", {arrow::large_utf8(), arrow::large_binary()},
                                     {cp::InputType(arrow::boolean())}, BinaryFilterInit, BinaryFilterExec,
                                     &g_stock_filter_large_bin));
  ARROW_RETURN_NOT_OK(RegisterVector(reg, "array_take", {arrow::large_utf8(), arrow::large_binary()},
                                     {cp::InputType(cp::match::Integer())}, BinaryTakeInit, BinaryTakeExec,
                                     &g_stock_take_large_bin));
  // round 4: fixed_size_list / list / large_list whose nested values are fixed-width and free of nulls (plugin/selection_nested.inc);
  // one stock kernel per type id (FSLFilterExec, ListFilterExec, LargeListFilterExec and their take twins)
  {
    const std::shared_ptr<arrow::DataType> f32 = arrow::float32();
    const struct { ValueType vt; StockKernel* filter; StockKernel* take; } nested[] = {
        {{arrow::fixed_size_list(f32, 4), Type::FIXED_SIZE_LIST}, &g_stock_filter_fsl, &g_stock_take_fsl},
        {{arrow::list(f32), Type::LIST}, &g_stock_filter_list, &g_stock_take_list},
        {{arrow::large_list(f32), Type::LARGE_LIST}, &g_stock_filter_large_list, &g_stock_take_large_list}};
    for (const auto& e : nested) {
      ARROW_RETURN_NOT_OK(RegisterVector(reg, "array_filter", {e.vt}, {cp::InputType(arrow::boolean())}, NestedFilterInit, NestedFilterExec, e.filter));
      ARROW_RETURN_NOT_OK(RegisterVector(reg, "array_take", {e.vt}, {cp::InputType(cp::match::Integer())}, NestedTakeInit, NestedTakeExec, e.take));
    }
  }
#define ARX_REGISTER_SORT(K, TYPE)                                                                           \
  ARROW_RETURN_NOT_OK(RegisterVector(reg, "array_sort_indices", {TYPE}, {}, SortInitT<K>, SortExecT<K>,         \
                                     &g_stock_sort[K], SortChunkedT<K>))
  ARX_REGISTER_SORT(ARX_KEY_UINT64, arrow::uint64());
  ARX_REGISTER_SORT(ARX_KEY_INT64, arrow::int64());
  ARX_REGISTER_SORT(ARX_KEY_UINT32, arrow::uint32());
  ARX_REGISTER_SORT(ARX_KEY_INT32, arrow::int32());
  ARX_REGISTER_SORT(ARX_KEY_FLOAT64, arrow::float64());
  ARX_REGISTER_SORT(ARX_KEY_FLOAT32, arrow::float32());
  ARX_REGISTER_SORT(6, arrow::date32());
  ARX_REGISTER_SORT(7, arrow::date64());
  ARX_REGISTER_SORT(8, ValueType(arrow::timestamp(arrow::TimeUnit::NANO), Type::TIMESTAMP));
  ARX_REGISTER_SORT(9, ValueType(arrow::duration(arrow::TimeUnit::NANO), Type::DURATION));
  ARX_REGISTER_SORT(10, ValueType(arrow::time32(arrow::TimeUnit::SECOND), Type::TIME32));
  ARX_REGISTER_SORT(11, ValueType(arrow::time64(arrow::TimeUnit::NANO), Type::TIME64));
  ARX_REGISTER_SORT(12, arrow::int8());
  ARX_REGISTER_SORT(13, arrow::uint8());
  ARX_REGISTER_SORT(14, arrow::int16());
  ARX_REGISTER_SORT(15, arrow::uint16());
  ARX_REGISTER_SORT(kSortSlotDecimal, ValueType(arrow::decimal128(20, 2), Type::DECIMAL128));
  ARX_REGISTER_SORT(kSortSlotUtf8, arrow::utf8());
  ARX_REGISTER_SORT(kSortSlotBinary, arrow::binary());
  ARX_REGISTER_SORT(kSortSlotBoolean, arrow::boolean());
  ARX_REGISTER_SORT(kSortSlotDictionary, ValueType(arrow::dictionary(arrow::int32(), arrow::utf8()), Type::DICTIONARY));
  ARX_REGISTER_SORT(kSortSlotLargeUtf8, arrow::large_utf8());
  ARX_REGISTER_SORT(kSortSlotLargeBinary, arrow::large_binary());
  ARX_REGISTER_SORT(kSortSlotStruct, ValueType(arrow::struct_({arrow::field("a", arrow::int64())}), Type::STRUCT));
#undef ARX_REGISTER_SORT
  // compare / arithmetic / divide: one kernel per (function, numeric type) (plugin/scalar.inc)
#define ARX_NUM_TYPES(X)                                                                                                     \
  X(int8_t, arrow::Int8Scalar, ARX_NUM_INT8, arrow::int8(), 0) X(uint8_t, arrow::UInt8Scalar, ARX_NUM_UINT8, arrow::uint8(), 1) \
  X(int16_t, arrow::Int16Scalar, ARX_NUM_INT16, arrow::int16(), 2) X(uint16_t, arrow::UInt16Scalar, ARX_NUM_UINT16, arrow::uint16(), 3) \
  X(int32_t, arrow::Int32Scalar, ARX_NUM_INT32, arrow::int32(), 4) X(uint32_t, arrow::UInt32Scalar, ARX_NUM_UINT32, arrow::uint32(), 5) \
  X(int64_t, arrow::Int64Scalar, ARX_NUM_INT64, arrow::int64(), 6) X(uint64_t, arrow::UInt64Scalar, ARX_NUM_UINT64, arrow::uint64(), 7) \
  X(float, arrow::FloatScalar, ARX_NUM_FLOAT32, arrow::float32(), 8) X(double, arrow::DoubleScalar, ARX_NUM_FLOAT64, arrow::float64(), 9)
#define ARX_REG_CMP_NUM(CT, ST, NUM, TYPE, TI)                                                                                \
  ARROW_RETURN_NOT_OK((RegisterScalarBinaryNP<OpCompare<CT, ST, NUM, ARX_CMP_EQUAL, 0 * 10 + TI>>(reg, "equal", TYPE)));              \
  ARROW_RETURN_NOT_OK((RegisterScalarBinaryNP<OpCompare<CT, ST, NUM, ARX_CMP_NOT_EQUAL, 1 * 10 + TI>>(reg, "not_equal", TYPE)));      \
  ARROW_RETURN_NOT_OK((RegisterScalarBinaryNP<OpCompare<CT, ST, NUM, ARX_CMP_GREATER, 2 * 10 + TI>>(reg, "greater", TYPE)));          \
  ARROW_RETURN_NOT_OK((RegisterScalarBinaryNP<OpCompare<CT, ST, NUM, ARX_CMP_GREATER_EQUAL, 3 * 10 + TI>>(reg, "greater_equal", TYPE))); \
  ARROW_RETURN_NOT_OK((RegisterScalarBinaryNP<OpCompare<CT, ST, NUM, ARX_CMP_LESS, 4 * 10 + TI>>(reg, "less", TYPE)));                \
  ARROW_RETURN_NOT_OK((RegisterScalarBinaryNP<OpCompare<CT, ST, NUM, ARX_CMP_LESS_EQUAL, 5 * 10 + TI>>(reg, "less_equal", TYPE)));
  ARX_NUM_TYPES(ARX_REG_CMP_NUM)
#undef ARX_REG_CMP_NUM
#define ARX_REG_ARITH_NUM(CT, ST, NUM, TYPE, TI)                                                                              \
  ARROW_RETURN_NOT_OK((RegisterScalarBinaryNP<OpArith<CT, ST, NUM, ARX_ARITH_ADD, false, 0 * 10 + TI>>(reg, "add", TYPE)));            \
  ARROW_RETURN_NOT_OK((RegisterScalarBinaryNP<OpArith<CT, ST, NUM, ARX_ARITH_SUBTRACT, false, 1 * 10 + TI>>(reg, "subtract", TYPE)));  \
  ARROW_RETURN_NOT_OK((RegisterScalarBinaryNP<OpArith<CT, ST, NUM, ARX_ARITH_MULTIPLY, false, 2 * 10 + TI>>(reg, "multiply", TYPE)));  \
  ARROW_RETURN_NOT_OK((RegisterScalarBinaryNP<OpArith<CT, ST, NUM, ARX_ARITH_ADD, true, 3 * 10 + TI>>(reg, "add_checked", TYPE)));     \
  ARROW_RETURN_NOT_OK((RegisterScalarBinaryNP<OpArith<CT, ST, NUM, ARX_ARITH_SUBTRACT, true, 4 * 10 + TI>>(reg, "subtract_checked", TYPE))); \
  ARROW_RETURN_NOT_OK((RegisterScalarBinaryNP<OpArith<CT, ST, NUM, ARX_ARITH_MULTIPLY, true, 5 * 10 + TI>>(reg, "multiply_checked", TYPE)));
  ARX_NUM_TYPES(ARX_REG_ARITH_NUM)
#undef ARX_REG_ARITH_NUM
#define ARX_REG_DIVIDE_NUM(CT, ST, NUM, TYPE, TI)                                                                             \
  ARROW_RETURN_NOT_OK((RegisterScalarBinaryNP<OpDivide<CT, ST, NUM, false, 0 * 10 + TI>>(reg, "divide", TYPE)));             \
  ARROW_RETURN_NOT_OK((RegisterScalarBinaryNP<OpDivide<CT, ST, NUM, true, 1 * 10 + TI>>(reg, "divide_checked", TYPE)));
  ARX_NUM_TYPES(ARX_REG_DIVIDE_NUM)
#undef ARX_REG_DIVIDE_NUM
#undef ARX_NUM_TYPES
  // the comparisons for temporal types: one kernel per (function, type / unit), matched by unit whatever the zone
  {
    using arrow::TimeUnit;
#define ARX_REG_CMP_TEMPORAL(CT, ST, NUM, PROBE, MATCH, TI)                                                                     \
  {                                                                                                                             \
    const ValueType vt(PROBE, MATCH);                                                                                           \
    ARROW_RETURN_NOT_OK((RegisterScalarBinaryNP<OpCompareTemporal<CT, ST, NUM, ARX_CMP_EQUAL, 0 * 14 + TI>>(reg, "equal", vt)));              \
    ARROW_RETURN_NOT_OK((RegisterScalarBinaryNP<OpCompareTemporal<CT, ST, NUM, ARX_CMP_NOT_EQUAL, 1 * 14 + TI>>(reg, "not_equal", vt)));      \
    ARROW_RETURN_NOT_OK((RegisterScalarBinaryNP<OpCompareTemporal<CT, ST, NUM, ARX_CMP_GREATER, 2 * 14 + TI>>(reg, "greater", vt)));          \
    ARROW_RETURN_NOT_OK((RegisterScalarBinaryNP<OpCompareTemporal<CT, ST, NUM, ARX_CMP_GREATER_EQUAL, 3 * 14 + TI>>(reg, "greater_equal", vt))); \
    ARROW_RETURN_NOT_OK((RegisterScalarBinaryNP<OpCompareTemporal<CT, ST, NUM, ARX_CMP_LESS, 4 * 14 + TI>>(reg, "less", vt)));                \
    ARROW_RETURN_NOT_OK((RegisterScalarBinaryNP<OpCompareTemporal<CT, ST, NUM, ARX_CMP_LESS_EQUAL, 5 * 14 + TI>>(reg, "less_equal", vt)));    \
  }
    ARX_REG_CMP_TEMPORAL(int64_t, arrow::TimestampScalar, ARX_NUM_INT64, arrow::timestamp(TimeUnit::SECOND), cp::InputType(cp::match::TimestampTypeUnit(TimeUnit::SECOND)), 0)
    ARX_REG_CMP_TEMPORAL(int64_t, arrow::TimestampScalar, ARX_NUM_INT64, arrow::timestamp(TimeUnit::MILLI), cp::InputType(cp::match::TimestampTypeUnit(TimeUnit::MILLI)), 1)
    ARX_REG_CMP_TEMPORAL(int64_t, arrow::TimestampScalar, ARX_NUM_INT64, arrow::timestamp(TimeUnit::MICRO), cp::InputType(cp::match::TimestampTypeUnit(TimeUnit::MICRO)), 2)
    ARX_REG_CMP_TEMPORAL(int64_t, arrow::TimestampScalar, ARX_NUM_INT64, arrow::timestamp(TimeUnit::NANO), cp::InputType(cp::match::TimestampTypeUnit(TimeUnit::NANO)), 3)
    ARX_REG_CMP_TEMPORAL(int64_t, arrow::DurationScalar, ARX_NUM_INT64, arrow::duration(TimeUnit::SECOND), cp::InputType(cp::match::DurationTypeUnit(TimeUnit::SECOND)), 4)
    ARX_REG_CMP_TEMPORAL(int64_t, arrow::DurationScalar, ARX_NUM_INT64, arrow::duration(TimeUnit::MILLI), cp::InputType(cp::match::DurationTypeUnit(TimeUnit::MILLI)), 5)
    ARX_REG_CMP_TEMPORAL(int64_t, arrow::DurationScalar, ARX_NUM_INT64, arrow::duration(TimeUnit::MICRO), cp::InputType(cp::match::DurationTypeUnit(TimeUnit::MICRO)), 6)
    ARX_REG_CMP_TEMPORAL(int64_t, arrow::DurationScalar, ARX_NUM_INT64, arrow::duration(TimeUnit::NANO), cp::InputType(cp::match::DurationTypeUnit(TimeUnit::NANO)), 7)
    ARX_REG_CMP_TEMPORAL(int32_t, arrow::Time32Scalar, ARX_NUM_INT32, arrow::time32(TimeUnit::SECOND), cp::InputType(cp::match::Time32TypeUnit(TimeUnit::SECOND)), 8)
    ARX_REG_CMP_TEMPORAL(int32_t, arrow::Time32Scalar, ARX_NUM_INT32, arrow::time32(TimeUnit::MILLI), cp::InputType(cp::match::Time32TypeUnit(TimeUnit::MILLI)), 9)
    ARX_REG_CMP_TEMPORAL(int64_t, arrow::Time64Scalar, ARX_NUM_INT64, arrow::time64(TimeUnit::MICRO), cp::InputType(cp::match::Time64TypeUnit(TimeUnit::MICRO)), 10)
    ARX_REG_CMP_TEMPORAL(int64_t, arrow::Time64Scalar, ARX_NUM_INT64, arrow::time64(TimeUnit::NANO), cp::InputType(cp::match::Time64TypeUnit(TimeUnit::NANO)), 11)
    ARX_REG_CMP_TEMPORAL(int32_t, arrow::Date32Scalar, ARX_NUM_INT32, arrow::date32(), cp::InputType(arrow::date32()), 12)
    ARX_REG_CMP_TEMPORAL(int64_t, arrow::Date64Scalar, ARX_NUM_INT64, arrow::date64(), cp::InputType(arrow::date64()), 13)
#undef ARX_REG_CMP_TEMPORAL
  }
  ARROW_RETURN_NOT_OK(RegisterBooleanNP(reg, "and_kleene", 2, KleeneExecNP<ARX_AND_KLEENE>, &g_stock_and_kleene));
  ARROW_RETURN_NOT_OK(RegisterBooleanNP(reg, "or_kleene", 2, KleeneExecNP<ARX_OR_KLEENE>, &g_stock_or_kleene));
  ARROW_RETURN_NOT_OK(RegisterBooleanNP(reg, "invert", 1, InvertExecNP, &g_stock_invert));
  for (const auto& names : {std::pair<const char*, const char*>{"filter", "array_filter"}, {"take", "array_take"}}) {
    ARROW_ASSIGN_OR_RAISE(auto stock, reg->GetFunction(names.first));
    ARROW_RETURN_NOT_OK(reg->AddFunction(
        std::make_shared<RocmSelectionMetaFunction>(names.first, std::move(stock), names.second), /*allow_overwrite=*/true));
  }
  {
    ARROW_ASSIGN_OR_RAISE(auto stock_sort, reg->GetFunction("sort_indices"));
    ARROW_RETURN_NOT_OK(reg->AddFunction(std::make_shared<RocmSortIndicesMetaFunction>(std::move(stock_sort)),
                                         /*allow_overwrite=*/true));
  }
  ARROW_RETURN_NOT_OK(RegisterRankFunctions(reg));   // rank / rank_quantile / select_k_unstable / partition_nth_indices (plugin/rank.inc)
  {
    ARROW_ASSIGN_OR_RAISE(auto stock_cast, reg->GetFunction("cast"));
    ARROW_RETURN_NOT_OK(reg->AddFunction(std::make_shared<RocmCastMetaFunction>(std::move(stock_cast)),
                                         /*allow_overwrite=*/true));
  }
  {
    ARROW_ASSIGN_OR_RAISE(auto fn, reg->GetFunction("hash_sum"));
    if (fn->kind() != cp::Function::HASH_AGGREGATE) return Status::Invalid("hash_sum is not a hash aggregate");
    auto* hfn = static_cast<cp::HashAggregateFunction*>(fn.get());
    // every integer width (the reference registers hash_sum for all of them, hash_aggregate_numeric.cc); the accumulator
    // — and the output — is int64 for the signed types and uint64 for the unsigned ones (aggregate_internal.h:41-58)
    // round 4: float32 / float64 — double accumulators fed in row order, as the reference's (arx_hash_sum_float_consume)
    for (const auto& value_type : {arrow::int8(), arrow::uint8(), arrow::int16(), arrow::uint16(), arrow::int32(), arrow::uint32(),
                                   arrow::int64(), arrow::uint64(), arrow::float32(), arrow::float64()}) {
      ARROW_ASSIGN_OR_RAISE(const cp::Kernel* k0, hfn->DispatchExact({value_type, arrow::uint32()}));
      cp::HashAggregateKernel copy = *static_cast<const cp::HashAggregateKernel*>(k0);
      // the stock signature's output resolver casts the kernel state to the reference's
      // GroupedAggregator (hash_aggregate_internal.h:88-91) — ours is not one: state the type
      copy.signature = cp::KernelSignature::Make({cp::InputType(value_type), cp::InputType(arrow::uint32())},
                                                 cp::OutputType(SumOutType(SumNumType(value_type->id()))));
      copy.init = HashSumInit;
      copy.resize = HashSumResize;
      copy.consume = HashSumConsume;
      copy.merge = HashSumMerge;
      copy.finalize = HashSumFinalize;
      ARROW_RETURN_NOT_OK(hfn->AddKernel(std::move(copy)));
    }
  }
  {
    // hash_sum of decimal128 (any precision / scale): 128-bit sums modulo 2^128 on the device (csrc/decimal.hip)
    ARROW_ASSIGN_OR_RAISE(auto fn, reg->GetFunction("hash_sum"));
    auto* hfn = static_cast<cp::HashAggregateFunction*>(fn.get());
    ARROW_ASSIGN_OR_RAISE(const cp::Kernel* k0, hfn->DispatchExact({arrow::decimal128(20, 2), arrow::uint32()}));
    cp::HashAggregateKernel copy = *static_cast<const cp::HashAggregateKernel*>(k0);
    copy.signature = cp::KernelSignature::Make({cp::InputType(Type::DECIMAL128), cp::InputType(arrow::uint32())}, cp::OutputType(ResolveDecimalSum));
    copy.init = HashSumInit;
    copy.resize = HashSumResize;
    copy.consume = HashSumConsume;
    copy.merge = HashSumMerge;
    copy.finalize = HashSumFinalize;
    ARROW_RETURN_NOT_OK(hfn->AddKernel(std::move(copy)));
  }
  // the other hash_* kernels the stock GroupByNode asks for (plugin/hash_aggregate_more.inc)
  ARROW_RETURN_NOT_OK(RegisterDenseAggregate<kDenseCount>(reg, "hash_count",
                                                          cp::InputType(std::make_shared<PhysicalValidityMatcher>()),
                                                          arrow::int64(), arrow::int64()));
  // min / max / mean of every integer width (narrow values are widened on the device; the extrema of uint64 are taken
  // on x + 2^63 read as int64, the order-preserving map)
  for (const auto& vt : {arrow::int8(), arrow::uint8(), arrow::int16(), arrow::uint16(), arrow::int32(), arrow::uint32(),
                         arrow::int64(), arrow::uint64()}) {
    ARROW_RETURN_NOT_OK(RegisterDenseAggregate<kDenseMin>(reg, "hash_min", cp::InputType(vt), vt, vt));
    ARROW_RETURN_NOT_OK(RegisterDenseAggregate<kDenseMax>(reg, "hash_max", cp::InputType(vt), vt, vt));
  }
  // round 4: float32 / float64 extrema (order keys in the same int64 state), the temporal types (their physical int32 /
  // int64), and hash_min_max (struct<min, max>) for all of them
  for (const auto& vt : {arrow::float32(), arrow::float64()}) {
    ARROW_RETURN_NOT_OK(RegisterDenseAggregate<kDenseMin>(reg, "hash_min", cp::InputType(vt), vt, vt));
    ARROW_RETURN_NOT_OK(RegisterDenseAggregate<kDenseMax>(reg, "hash_max", cp::InputType(vt), vt, vt));
  }
  for (const auto& vt : {arrow::date32(), arrow::date64(), arrow::time32(arrow::TimeUnit::SECOND), arrow::time64(arrow::TimeUnit::MICRO),
                         arrow::timestamp(arrow::TimeUnit::SECOND)}) {
    ARROW_RETURN_NOT_OK(RegisterDenseAggregate<kDenseMin>(reg, "hash_min", cp::InputType(vt->id()), cp::OutputType(ResolveFirstType), vt));
    ARROW_RETURN_NOT_OK(RegisterDenseAggregate<kDenseMax>(reg, "hash_max", cp::InputType(vt->id()), cp::OutputType(ResolveFirstType), vt));
    ARROW_RETURN_NOT_OK(RegisterDenseAggregate<kDenseMinMax>(reg, "hash_min_max", cp::InputType(vt->id()), cp::OutputType(ResolveMinMaxStruct), vt));
  }
  for (const auto& vt : {arrow::int8(), arrow::uint8(), arrow::int16(), arrow::uint16(), arrow::int32(), arrow::uint32(),
                         arrow::int64(), arrow::uint64(), arrow::float32(), arrow::float64()}) {
    ARROW_RETURN_NOT_OK(RegisterDenseAggregate<kDenseMinMax>(reg, "hash_min_max", cp::InputType(vt), cp::OutputType(ResolveMinMaxStruct), vt));
  }
  for (const auto& vt : {arrow::int8(), arrow::uint8(), arrow::int16(), arrow::uint16(), arrow::int32(), arrow::uint32(),
                         arrow::uint64()}) {
    ARROW_RETURN_NOT_OK(RegisterDenseAggregate<kDenseMean>(reg, "hash_mean", cp::InputType(vt), arrow::float64(), vt));
  }
  ARROW_RETURN_NOT_OK(RegisterDenseAggregate<kDenseMean>(reg, "hash_mean", cp::InputType(arrow::int64()), arrow::float64(),
                                                         arrow::int64()));   // (last: its stock kernel is the one kept for host batches)
  {
    // hash_mean of float32 / float64: the hash_sum vtable with a dividing Finalize (the integer types' hash_mean keeps its
    // own vtable, plugin/hash_aggregate_more.inc: it has to decide whether its double sums are exact)
    ARROW_ASSIGN_OR_RAISE(auto fn, reg->GetFunction("hash_mean"));
    auto* hfn = static_cast<cp::HashAggregateFunction*>(fn.get());
    for (const auto& value_type : {arrow::float32(), arrow::float64(), arrow::decimal128(20, 2)}) {
      ARROW_ASSIGN_OR_RAISE(const cp::Kernel* k0, hfn->DispatchExact({value_type, arrow::uint32()}));
      cp::HashAggregateKernel copy = *static_cast<const cp::HashAggregateKernel*>(k0);
      if (value_type->id() == Type::DECIMAL128) {   // any precision / scale; the mean keeps the input's type
        copy.signature = cp::KernelSignature::Make({cp::InputType(Type::DECIMAL128), cp::InputType(arrow::uint32())}, cp::OutputType(ResolveFirstType));
      } else {
        copy.signature = cp::KernelSignature::Make({cp::InputType(value_type), cp::InputType(arrow::uint32())}, cp::OutputType(arrow::float64()));
      }
      copy.init = HashMeanFloatInit;
      copy.resize = HashSumResize;
      copy.consume = HashSumConsume;
      copy.merge = HashSumMerge;
      copy.finalize = HashSumFinalize;
      ARROW_RETURN_NOT_OK(hfn->AddKernel(std::move(copy)));
    }
  }
  ARROW_RETURN_NOT_OK(RegisterBoolAggregate<false>(reg, "hash_any"));
  ARROW_RETURN_NOT_OK(RegisterBoolAggregate<true>(reg, "hash_all"));
  // hash vector kernels on device-resident arrays through the device Grouper (plugin/vector_hash.inc)
  ARROW_RETURN_NOT_OK(RegisterHashVector<kHashUnique>(reg, "unique", &g_stock_unique, &g_stock_unique_finalize));
  ARROW_RETURN_NOT_OK(RegisterHashVector<kHashValueCounts>(reg, "value_counts", &g_stock_value_counts, &g_stock_value_counts_finalize));
  ARROW_RETURN_NOT_OK(RegisterHashVector<kHashDictEncode>(reg, "dictionary_encode", &g_stock_dict_encode, &g_stock_dict_encode_finalize));
  {
    ARROW_ASSIGN_OR_RAISE(auto stock_drop_null, reg->GetFunction("drop_null"));
    ARROW_RETURN_NOT_OK(reg->AddFunction(std::make_shared<RocmDropNullMetaFunction>(std::move(stock_drop_null)), /*allow_overwrite=*/true));
  }
  ARROW_RETURN_NOT_OK(RegisterIndicesNonZero(reg));
  ARROW_RETURN_NOT_OK(RegisterDeviceCountAny(reg));   // (count of any physical type; the integer types' kernels come after it)
  ARROW_RETURN_NOT_OK(RegisterDeviceAggregate<kAggSum>(reg, "sum"));
  ARROW_RETURN_NOT_OK(RegisterDeviceAggregate<kAggCount>(reg, "count"));
  ARROW_RETURN_NOT_OK(RegisterDeviceAggregate<kAggMinMax>(reg, "min_max"));
  ARROW_RETURN_NOT_OK(RegisterDeviceAggregate<kAggMin>(reg, "min"));
  ARROW_RETURN_NOT_OK(RegisterDeviceAggregate<kAggMax>(reg, "max"));
  ARROW_RETURN_NOT_OK(RegisterDeviceAggregate<kAggMean>(reg, "mean"));
  ARROW_RETURN_NOT_OK(RegisterCoalesce(reg));   // coalesce(values, fill) = fill_null on device arrays (plugin/coalesce.inc)
  // is_valid / is_null / true_unless_null answer from the validity bitmap in HBM (the reference's kernels see none and
  // answer "no nulls" for a device-resident array) — plugin/validity.inc
  ARROW_RETURN_NOT_OK(RegisterValidityNP<kIsValid>(reg, "is_valid"));
  ARROW_RETURN_NOT_OK(RegisterValidityNP<kIsNull>(reg, "is_null"));
  ARROW_RETURN_NOT_OK(RegisterValidityNP<kTrueUnlessNull>(reg, "true_unless_null"));
  // is_in / index_in against a device hash table of the value set (plugin/set_lookup.inc)
  ARROW_RETURN_NOT_OK(RegisterSetLookup(reg, "is_in", false));
  ARROW_RETURN_NOT_OK(RegisterSetLookup(reg, "index_in", true));
  // match_substring / starts_with / ends_with with a literal pattern on utf8 / binary columns (plugin/match_substring.inc)
  ARROW_RETURN_NOT_OK(RegisterMatchSubstring(reg, "match_substring", ARX_MATCH_SUBSTRING, kFnMatchSubstring));
  ARROW_RETURN_NOT_OK(RegisterMatchSubstring(reg, "starts_with", ARX_MATCH_STARTS_WITH, kFnStartsWith));
  ARROW_RETURN_NOT_OK(RegisterMatchSubstring(reg, "ends_with", ARX_MATCH_ENDS_WITH, kFnEndsWith));
  ARROW_RETURN_NOT_OK(RegisterIfElse(reg));   // if_else(cond, left, right) of boolean and the fixed-width types (plugin/if_else.inc)
  ARROW_RETURN_NOT_OK(RegisterTemporal(reg));   // year .. iso_week, hour .. nanosecond of dates, timestamps and times (plugin/temporal.inc)
  ARROW_RETURN_NOT_OK(RegisterStringSlice(reg));   // binary_length, utf8_length, binary_slice, utf8_slice_codeunits (plugin/string_slice.inc)
  ARROW_RETURN_NOT_OK(RegisterStringTrim(reg));    // the twelve {ascii,utf8}_{,l,r}trim{,_whitespace} (plugin/string_trim.inc)
  ARROW_RETURN_NOT_OK(RegisterStringCompare(reg));   // equal .. less_equal of utf8 / binary and their large forms (plugin/string_compare.inc)
  ARROW_RETURN_NOT_OK(RegisterStringReplace(reg));   // replace_substring of utf8 / binary and their large forms (plugin/string_replace.inc)
  ARROW_RETURN_NOT_OK(RegisterStringJoin(reg));   // binary_join_element_wise of utf8 / binary and their large forms (plugin/string_join.inc)
  ARROW_RETURN_NOT_OK(RegisterUnaryArith(reg));   // negate .. trunc, round, round_to_multiple of the numeric types (plugin/unary_arith.inc)
  ARROW_RETURN_NOT_OK(RegisterCaseWhen(reg));   // case_when(cond struct, values ..., [else]) of boolean and the fixed-width types (plugin/case_when.inc)
  // min_element_wise / max_element_wise of the numeric types and the physically-integer temporal ones (plugin/element_wise.inc)
  ARROW_RETURN_NOT_OK(RegisterElementWise(reg, "min_element_wise", ARX_ELEMENT_WISE_MIN, kFnMinElementWise));
  ARROW_RETURN_NOT_OK(RegisterElementWise(reg, "max_element_wise", ARX_ELEMENT_WISE_MAX, kFnMaxElementWise));
  // the reference's kernels of the functions extended above refuse device-resident arrays instead of reading them
  ARROW_RETURN_NOT_OK(InstallDeviceGuards(reg, stock_kernel_counts));
  ARROW_RETURN_NOT_OK(RefreshMinMaxKernels(reg));   // (the guards re-added kernels: pointers into min_max's list moved)
  {
    const Status st = ac::default_exec_factory_registry()->AddFactory("aggregate_rocm", MakeAggregateRocm);
    if (!st.ok() && !st.IsKeyError()) return st;
  }
  {
    const Status st = ac::default_exec_factory_registry()->AddFactory("order_by_rocm", RocmOrderByNode::Make);
    if (!st.ok() && !st.IsKeyError()) return st;
  }
  {
    const Status st = ac::default_exec_factory_registry()->AddFactory("hashjoin_rocm", RocmHashJoinNode::Make);
    if (!st.ok() && !st.IsKeyError()) return st;
  }
  {
    const Status st = ac::default_exec_factory_registry()->AddFactory("table_source_rocm", RocmTableSourceNode::Make);
    if (!st.ok() && !st.IsKeyError()) return st;
  }
  {
    const Status st = ac::default_exec_factory_registry()->AddFactory("coalesce_rocm", RocmCoalesceNode::Make);
    if (!st.ok() && !st.IsKeyError()) return st;
  }
  {
    // the guard in front of the reference's CPU Grouper (plugin/acero_override.inc); a registry whose layout is not
    // recognised stays untouched (arrow_amd_plugin_acero_guard() says which)
    const Status st = OverrideAceroFactories(0);
    g_acero_guard_installed.store(st.ok());
  }
  return Status::OK();
}

std::once_flag g_once;
Status g_register_status;

// hash_sum HashAggregateKernel vtable over dense group ids.
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- hash_sum(int64, uint32)
// The HashAggregateKernel vtable (compute/kernel.h:720-769) of
// GroupedReducingAggregator<Int64Type,GroupedSumImpl> (hash_aggregate_numeric.cc:44-187) with the
// per-group state in HBM.  Acero's GroupByNode drives it unchanged
// (acero/groupby_aggregate_node.cc:210-337): resize after every Grouper::Consume, consume with
// the dense uint32 group ids, merge thread-local states through a group_id_mapping, finalize.
// value types of the hash_sum vtable: every integer width.  GroupedSumImpl accumulates int8 .. int64 in int64 and
// uint8 .. uint64 in uint64 (FindAccumulatorType, aggregate_internal.h:41-58); both wrap modulo 2^64, so ONE int64
// accumulator per group serves all of them — narrow values are sign- / zero-extended on the device first
// (arx_cast_numeric) and the output type follows the signedness.
constexpr int kNumDec128 = 64;   // (not an ARX_NUM_* id: decimal128 values, 16 bytes)
int SumNumType(Type::type id) {
  switch (id) {
    case Type::INT8: return ARX_NUM_INT8;
    case Type::UINT8: return ARX_NUM_UINT8;
    case Type::INT16: return ARX_NUM_INT16;
    case Type::UINT16: return ARX_NUM_UINT16;
    case Type::INT32: return ARX_NUM_INT32;
    case Type::UINT32: return ARX_NUM_UINT32;
    case Type::INT64: return ARX_NUM_INT64;
    case Type::UINT64: return ARX_NUM_UINT64;
    // round 4: float32 / float64 — a DOUBLE accumulator per group, fed in row order (arx_hash_sum_float_consume)
    case Type::FLOAT: return ARX_NUM_FLOAT32;
    case Type::DOUBLE: return ARX_NUM_FLOAT64;
    // round 4: decimal128 — a 128-bit sum per group modulo 2^128 (arx_hash_sum_dec128_*); hash_sum only
    case Type::DECIMAL128: return kNumDec128;
    default: return -1;
  }
}
bool SumNumIsFloat(int num_type) { return num_type == ARX_NUM_FLOAT32 || num_type == ARX_NUM_FLOAT64; }
int SumNumWidth(int num_type) {       // (integer ARX_NUM_* ids: the width doubles every two ids)
  if (num_type == kNumDec128) return 16;
  return SumNumIsFloat(num_type) ? (num_type == ARX_NUM_FLOAT32 ? 4 : 8) : 1 << (num_type >> 1);
}
bool SumNumUnsigned(int num_type) { return num_type < ARX_NUM_FLOAT32 && (num_type & 1) != 0; }
// FindAccumulatorType, aggregate_internal.h:41-58; a decimal keeps its scale and takes the largest precision
// (WidenDecimalToMaxPrecision, hash_aggregate_numeric.cc:165-167)
std::shared_ptr<arrow::DataType> SumOutType(int num_type, const arrow::DataType* in_type = nullptr) {
  if (num_type == kNumDec128) {
    return arrow::decimal128(38, in_type != nullptr ? static_cast<const arrow::Decimal128Type&>(*in_type).scale() : 0);
  }
  return SumNumIsFloat(num_type) ? arrow::float64() : (SumNumUnsigned(num_type) ? arrow::uint64() : arrow::int64());
}
arrow::Result<arrow::TypeHolder> ResolveDecimalSum(cp::KernelContext*, const std::vector<arrow::TypeHolder>& types) {
  return arrow::TypeHolder(SumOutType(kNumDec128, types[0].type));
}

// an integer scalar's value as the 64 bits the accumulator adds
arrow::Result<int64_t> IntegerScalarBits(const arrow::Scalar& sc) {
  switch (sc.type->id()) {
    case Type::INT8: return static_cast<int64_t>(static_cast<const arrow::Int8Scalar&>(sc).value);
    case Type::UINT8: return static_cast<int64_t>(static_cast<const arrow::UInt8Scalar&>(sc).value);
    case Type::INT16: return static_cast<int64_t>(static_cast<const arrow::Int16Scalar&>(sc).value);
    case Type::UINT16: return static_cast<int64_t>(static_cast<const arrow::UInt16Scalar&>(sc).value);
    case Type::INT32: return static_cast<int64_t>(static_cast<const arrow::Int32Scalar&>(sc).value);
    case Type::UINT32: return static_cast<int64_t>(static_cast<const arrow::UInt32Scalar&>(sc).value);
    case Type::INT64: return static_cast<const arrow::Int64Scalar&>(sc).value;
    case Type::UINT64: return static_cast<int64_t>(static_cast<const arrow::UInt64Scalar&>(sc).value);
    default: return Status::NotImplemented("arrow_amd: scalar of type ", sc.type->ToString());
  }
}

// A device span of `num_type` integers -> the dense 64-bit span the sum / min-max kernels take (validity re-based to bit 0).
Status WidenTo64(int num_type, hipStream_t st, ArxSpan* dv) {
  if (num_type == ARX_NUM_INT64 || num_type == ARX_NUM_UINT64 || dv->length == 0) return Status::OK();
  const int64_t n = dv->length;
  void *wide = nullptr, *ws = nullptr;
  // (slots no consume path of the hash_* vtables uses for anything else)
  ARROW_RETURN_NOT_OK(t_scratch.Get(kBinWs, static_cast<size_t>(n) * 8 + 16, &wide));
  ARROW_RETURN_NOT_OK(t_scratch.Get(kCounter, 64, &ws));
  ARROW_RETURN_NOT_OK(FromArx(arx_cast_numeric(dv, num_type, SumNumUnsigned(num_type) ? ARX_NUM_UINT64 : ARX_NUM_INT64,
                                               /*allow_int_overflow=*/1, /*allow_float_truncate=*/1, ws, 64, wide, st)));
  const void* validity = nullptr;
  if (dv->validity != nullptr && dv->null_count != 0) {
    void* bits = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(kFlag, static_cast<size_t>((n + 63) / 64) * 8 + 16, &bits));
    ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy(dv->validity, dv->offset, n, bits, st)));
    validity = bits;
  }
  *dv = ArxSpan{validity, wide, 0, n, dv->null_count};
  return Status::OK();
}

// uint64 values whose ORDER matters (min / max, and the bound of mean): y = x + 2^63 (mod 2^64) read as int64 is the
// order-preserving map of uint64 onto int64.  A device span of uint64 -> a dense span of those y (validity re-based to
// bit 0), in the scratch slots WidenTo64 uses for the narrow types (a column is either narrow or 64-bit).
constexpr uint64_t kUInt64Half = uint64_t(1) << 63;
Status FlipUInt64(hipStream_t st, ArxSpan* dv) {
  const int64_t n = dv->length;
  if (n == 0) return Status::OK();
  void* shifted = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kBinWs, static_cast<size_t>(n) * 8 + 16, &shifted));
  ARROW_RETURN_NOT_OK(FromArx(arx_arith_numeric(ARX_ARITH_ADD, 0, ARX_NUM_UINT64, static_cast<const uint64_t*>(dv->data) + dv->offset,
                                                nullptr, nullptr, 0, nullptr, &kUInt64Half, nullptr, 0, n, shifted, nullptr, st)));
  const void* validity = nullptr;
  if (dv->validity != nullptr && dv->null_count != 0) {
    void* bits = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(kFlag, static_cast<size_t>((n + 63) / 64) * 8 + 16, &bits));
    ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy(dv->validity, dv->offset, n, bits, st)));
    validity = bits;
  }
  *dv = ArxSpan{validity, shifted, 0, n, dv->null_count};
  return Status::OK();
}

struct DeviceSumState : public cp::KernelState {
  int num_type = ARX_NUM_INT64;
  bool mean = false;       // hash_mean of float32 / float64: the same state, Finalize divides (GroupedMeanImpl::DoMean)
  cp::ScalarAggregateOptions options;
  int64_t num_groups = 0;
  int64_t capacity = 0;
  int64_t* sums = nullptr;
  int64_t* sums_hi = nullptr;      // decimal128: the high words (sums = the low words)
  std::shared_ptr<arrow::DataType> out_type;
  int64_t* counts = nullptr;
  uint32_t* null_seen = nullptr;
  ~DeviceSumState() override {
    if (sums_hi) (void)hipFree(sums_hi);
    if (sums) (void)hipFree(sums);
    if (counts) (void)hipFree(counts);
    if (null_seen) (void)hipFree(null_seen);
  }
};

arrow::Result<std::unique_ptr<cp::KernelState>> HashSumInit(cp::KernelContext*,
                                                            const cp::KernelInitArgs& args) {
  auto state = std::make_unique<DeviceSumState>();
  if (!args.inputs.empty() && args.inputs[0].type != nullptr) {
    const int t = SumNumType(args.inputs[0].type->id());
    if (t < 0) return Status::NotImplemented("arrow_amd: hash_sum of ", args.inputs[0].type->ToString());
    state->num_type = t;
    state->out_type = SumOutType(t, args.inputs[0].type);
  }
  if (args.options != nullptr) {
    state->options = *static_cast<const cp::ScalarAggregateOptions*>(args.options);
  }
  return state;
}

arrow::Result<std::unique_ptr<cp::KernelState>> HashMeanFloatInit(cp::KernelContext* ctx, const cp::KernelInitArgs& args) {
  ARROW_ASSIGN_OR_RAISE(auto state, HashSumInit(ctx, args));
  auto* s = static_cast<DeviceSumState*>(state.get());
  if (!SumNumIsFloat(s->num_type) && s->num_type != kNumDec128) {
    return Status::NotImplemented("arrow_amd: this hash_mean kernel takes float32 / float64 / decimal128 values");
  }
  s->mean = true;
  // GroupedMeanImpl: PromoteDecimal() is false — a decimal mean keeps the input's type (hash_aggregate_numeric.cc:432-437)
  if (s->num_type == kNumDec128 && !args.inputs.empty()) s->out_type = args.inputs[0].GetSharedPtr();
  return state;
}

// GroupedMeanImpl::DoMean for decimals (hash_aggregate_numeric.cc:367-380): the 128-bit sum divided by the count, truncating
// (BasicDecimal128::Divide), then rounded half away from zero by the remainder.  values: 16-byte little-endian sums, replaced
// by the means in place — on the HOST: the column is on its way there, one division per group.  Finish (:402-424) divides
// EVERY group whose count reaches min_count: with min_count = 0 a group without a valid value is divided by zero, and the
// reference's BasicDecimal128::Divide fails the whole Finalize with Invalid("Division by 0 in Decimal") — so does this.
Status DecimalMeansInPlace(uint8_t* values, const int64_t* counts, int64_t g, uint32_t min_count) {
  for (int64_t i = 0; i < g; ++i) {
    if (counts[i] < static_cast<int64_t>(min_count)) continue;     // (null: Finish writes a zero there)
    if (counts[i] == 0) return Status::Invalid("Division by 0 in Decimal");
    uint64_t lo, hi;
    std::memcpy(&lo, values + 16 * i, 8);
    std::memcpy(&hi, values + 16 * i + 8, 8);
    const __int128 reduced = static_cast<__int128>((static_cast<unsigned __int128>(hi) << 64) | lo);
    const __int128 c = counts[i];
    __int128 q = reduced / c, r = reduced % c;
    if (r < 0) r = -r;
    if (r * 2 >= c) q += reduced >= 0 ? 1 : -1;
    lo = static_cast<uint64_t>(static_cast<unsigned __int128>(q));
    hi = static_cast<uint64_t>(static_cast<unsigned __int128>(q) >> 64);
    std::memcpy(values + 16 * i, &lo, 8);
    std::memcpy(values + 16 * i + 8, &hi, 8);
  }
  return Status::OK();
}

template <typename T>
Status GrowDevice(T** ptr, int64_t old_n, int64_t new_cap, hipStream_t st) {
  T* fresh = nullptr;
  HIP_RETURN_NOT_OK(hipMalloc(reinterpret_cast<void**>(&fresh), static_cast<size_t>(new_cap) * sizeof(T)));
  HIP_RETURN_NOT_OK(hipMemsetAsync(fresh, 0, static_cast<size_t>(new_cap) * sizeof(T), st));
  if (old_n > 0) {
    HIP_RETURN_NOT_OK(hipMemcpyAsync(fresh, *ptr, static_cast<size_t>(old_n) * sizeof(T),
                                     hipMemcpyDeviceToDevice, st));
  }
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  if (*ptr) HIP_RETURN_NOT_OK(hipFree(*ptr));
  *ptr = fresh;
  return Status::OK();
}

// Resize (:61-68): new groups start at sum 0 / count 0 / no null seen.
Status HashSumResize(cp::KernelContext* ctx, int64_t new_num_groups) {
  auto* s = static_cast<DeviceSumState*>(ctx->state());
  if (new_num_groups > s->capacity) {
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    const int64_t cap = std::max<int64_t>({new_num_groups, 2 * s->capacity, 1024});
    ARROW_RETURN_NOT_OK(GrowDevice(&s->sums, s->num_groups, cap, st));
    if (s->num_type == kNumDec128) ARROW_RETURN_NOT_OK(GrowDevice(&s->sums_hi, s->num_groups, cap, st));
    ARROW_RETURN_NOT_OK(GrowDevice(&s->counts, s->num_groups, cap, st));
    ARROW_RETURN_NOT_OK(GrowDevice(&s->null_seen, s->num_groups, cap, st));
    s->capacity = cap;
  }
  s->num_groups = new_num_groups;
  return Status::OK();
}

// Consume (:70-83): batch = {values (array | scalar), group ids (uint32 array)}.
Status HashSumConsume(cp::KernelContext* ctx, const cp::ExecSpan& batch) {
  auto* s = static_cast<DeviceSumState*>(ctx->state());
  const ArraySpan& gids = batch[1].array;
  const int64_t n = gids.length;
  if (n == 0) return Status::OK();
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  ArxSpan dg{};
  if (OnRocm(gids)) {
    ARROW_RETURN_NOT_OK(DeviceSpan(gids, &dg));
  } else {
    ARROW_RETURN_NOT_OK(Upload(gids, 4, kArg2, kArg2Validity, st, &dg));
  }
  const uint32_t* d_gids = static_cast<const uint32_t*>(dg.data) + dg.offset;
  ArxSpan dv{};
  int is_scalar = 0;
  int64_t scalar_value = 0;
  if (s->num_type == kNumDec128) {
    uint64_t scalar_lo = 0, scalar_hi = 0;
    if (batch[0].is_array()) {
      if (OnRocm(batch[0].array)) {
        ARROW_RETURN_NOT_OK(DeviceSpan(batch[0].array, &dv));
      } else {
        ARROW_RETURN_NOT_OK(Upload(batch[0].array, 16, kValues, kValidity, st, &dv));
      }
    } else {
      const arrow::Scalar& sc = *batch[0].scalar;
      is_scalar = 1;
      dv.length = n;
      dv.null_count = sc.is_valid ? 0 : n;
      if (sc.is_valid) {
        const arrow::Decimal128& d = static_cast<const arrow::Decimal128Scalar&>(sc).value;
        scalar_lo = d.low_bits();
        scalar_hi = static_cast<uint64_t>(d.high_bits());
      }
    }
    ARROW_RETURN_NOT_OK(FromArx(arx_hash_sum_dec128_consume(&dv, is_scalar, scalar_lo, scalar_hi, d_gids, n, reinterpret_cast<uint64_t*>(s->sums),
                                                            reinterpret_cast<uint64_t*>(s->sums_hi), s->counts, s->null_seen, st)));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    CountGpu(kFnHashSum);
    return Status::OK();
  }
  if (SumNumIsFloat(s->num_type)) {
    // float32 / float64: the reference adds every row to its group's double in row order — so does the device
    // (stable sort by group id, one walker per group; arx_hash_sum_float_consume)
    double scalar_double = 0.0;
    if (batch[0].is_array()) {
      if (OnRocm(batch[0].array)) {
        ARROW_RETURN_NOT_OK(DeviceSpan(batch[0].array, &dv));
      } else {
        ARROW_RETURN_NOT_OK(Upload(batch[0].array, SumNumWidth(s->num_type), kValues, kValidity, st, &dv));
      }
    } else {
      const arrow::Scalar& sc = *batch[0].scalar;
      is_scalar = 1;
      dv.length = n;
      dv.null_count = sc.is_valid ? 0 : n;
      if (sc.is_valid) {
        scalar_double = sc.type->id() == Type::FLOAT ? static_cast<double>(static_cast<const arrow::FloatScalar&>(sc).value)
                                                     : static_cast<const arrow::DoubleScalar&>(sc).value;
      }
    }
    const size_t fws_bytes = arx_hash_sum_float_workspace_bytes(n);
    void* fws = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(kWs, fws_bytes + 256, &fws));
    ARROW_RETURN_NOT_OK(FromArx(arx_hash_sum_float_consume(&dv, s->num_type, is_scalar, scalar_double, d_gids, n, fws, fws_bytes + 256,
                                                           reinterpret_cast<double*>(s->sums), s->counts, s->null_seen, st)));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    CountGpu(kFnHashSum);
    return Status::OK();
  }
  if (batch[0].is_array()) {
    if (OnRocm(batch[0].array)) {   // a device-resident value column under a CPU Grouper: no staging over PCIe
      ARROW_RETURN_NOT_OK(DeviceSpan(batch[0].array, &dv));
    } else {
      ARROW_RETURN_NOT_OK(Upload(batch[0].array, SumNumWidth(s->num_type), kValues, kValidity, st, &dv));
    }
    ARROW_RETURN_NOT_OK(WidenTo64(s->num_type, st, &dv));   // (int8 .. uint32: sign- / zero-extended on the device)
  } else {
    const arrow::Scalar& sc = *batch[0].scalar;
    is_scalar = 1;
    dv.length = n;
    dv.null_count = sc.is_valid ? 0 : n;
    if (sc.is_valid) {
      ARROW_ASSIGN_OR_RAISE(scalar_value, IntegerScalarBits(sc));
    }
  }
  // large batches: partition by group id + LDS aggregation (needs scratch); Acero's 32K-row batches stay below the
  // library's threshold and keep the per-row atomics
  const size_t ws_bytes = arx_hash_sum_consume_workspace_bytes(n, s->num_groups);
  void* ws = nullptr;
  if (ws_bytes > 0 && n >= (int64_t(1) << 17)) {
    ARROW_RETURN_NOT_OK(t_scratch.Get(kWs, ws_bytes + 256, &ws));
    ws = Align256(ws);
  }
  ARROW_RETURN_NOT_OK(FromArx(arx_hash_sum_i64_consume_ws(&dv, is_scalar, scalar_value, d_gids, n, s->num_groups, s->sums,
                                                          s->counts, s->null_seen, ws, ws != nullptr ? ws_bytes : 0, st)));
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  CountGpu(kFnHashSum);
  return Status::OK();
}

// Merge (:85-107).
Status HashSumMerge(cp::KernelContext* ctx, cp::KernelState&& other_state, const ArrayData& mapping) {
  auto* s = static_cast<DeviceSumState*>(ctx->state());
  auto* other = static_cast<DeviceSumState*>(&other_state);
  const int64_t g = mapping.length;
  if (g == 0) return Status::OK();
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  void* d_map = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kArg2, static_cast<size_t>(g) * 4 + 16, &d_map));
  HIP_RETURN_NOT_OK(hipMemcpyAsync(d_map, mapping.GetValues<uint32_t>(1), static_cast<size_t>(g) * 4,
                                   hipMemcpyHostToDevice, st));
  if (s->num_type == kNumDec128) {
    ARROW_RETURN_NOT_OK(FromArx(arx_hash_sum_dec128_merge(reinterpret_cast<uint64_t*>(s->sums), reinterpret_cast<uint64_t*>(s->sums_hi), s->counts,
                                                          s->null_seen, reinterpret_cast<const uint64_t*>(other->sums),
                                                          reinterpret_cast<const uint64_t*>(other->sums_hi), other->counts, other->null_seen,
                                                          static_cast<const uint32_t*>(d_map), g, st)));
  } else if (SumNumIsFloat(s->num_type)) {
    ARROW_RETURN_NOT_OK(FromArx(arx_hash_sum_f64_merge(reinterpret_cast<double*>(s->sums), s->counts, s->null_seen,
                                                       reinterpret_cast<const double*>(other->sums), other->counts, other->null_seen,
                                                       static_cast<const uint32_t*>(d_map), g, st)));
  } else {
    ARROW_RETURN_NOT_OK(FromArx(arx_hash_sum_i64_merge(s->sums, s->counts, s->null_seen, other->sums,
                                                       other->counts, other->null_seen,
                                                       static_cast<const uint32_t*>(d_map), g, st)));
  }
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
  return Status::OK();
}

// Finalize (:130-152) + Finish (:109-128).
Status HashSumFinalize(cp::KernelContext* ctx, arrow::Datum* out) {
  auto* s = static_cast<DeviceSumState*>(ctx->state());
  const int64_t g = s->num_groups;
  arrow::MemoryPool* pool = ctx->memory_pool();
  std::shared_ptr<Buffer> values;
  if (g == 0) {
    ARROW_ASSIGN_OR_RAISE(values, arrow::AllocateBuffer(0, pool));
  }
  std::shared_ptr<Buffer> bitmap;
  int64_t null_count = 0;
  if (g > 0) {
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    void *d_bits = nullptr, *d_counter = nullptr;
    const size_t words = static_cast<size_t>((g + 63) / 64);
    ARROW_RETURN_NOT_OK(t_scratch.Get(kOutValidity, words * 8 + 16, &d_bits));
    ARROW_RETURN_NOT_OK(t_scratch.Get(kCounter, 64, &d_counter));
    HIP_RETURN_NOT_OK(hipMemsetAsync(d_counter, 0, 8, st));
    ARROW_RETURN_NOT_OK(FromArx(arx_hash_sum_i64_finalize(s->counts, s->null_seen, g,
                                                          s->options.skip_nulls ? 1 : 0,
                                                          s->options.min_count, d_bits,
                                                          static_cast<int64_t*>(d_counter), st)));
    ARROW_ASSIGN_OR_RAISE(bitmap, arrow::AllocateBitmap(g, pool));
    int64_t valid_count = 0;
    const void* column = s->sums;
    if (s->mean && s->num_type != kNumDec128) {
      void* d_means = nullptr;
      ARROW_RETURN_NOT_OK(t_scratch.Get(kOutData, static_cast<size_t>(g) * 8 + 16, &d_means));
      ARROW_RETURN_NOT_OK(FromArx(arx_hash_mean_f64_finalize(reinterpret_cast<const double*>(s->sums), s->counts, g,
                                                             static_cast<double*>(d_means), st)));
      column = d_means;
    }
    int64_t out_width = 8;
    if (s->num_type == kNumDec128) {
      void* d_packed = nullptr;
      ARROW_RETURN_NOT_OK(t_scratch.Get(kOutData, static_cast<size_t>(g) * 16 + 16, &d_packed));
      ARROW_RETURN_NOT_OK(FromArx(arx_dec128_pack(reinterpret_cast<const uint64_t*>(s->sums), reinterpret_cast<const uint64_t*>(s->sums_hi), g,
                                                  d_packed, st)));
      column = d_packed;
      out_width = 16;
    }
    ARROW_ASSIGN_OR_RAISE(values, ColumnToHost(column, g * out_width, pool, st));
    std::vector<int64_t> host_counts;
    if (s->mean && s->num_type == kNumDec128) {
      host_counts.resize(static_cast<size_t>(g));
      HIP_RETURN_NOT_OK(hipMemcpyAsync(host_counts.data(), s->counts, static_cast<size_t>(g) * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_RETURN_NOT_OK(hipMemcpyAsync(bitmap->mutable_data(), d_bits,
                                     static_cast<size_t>(arrow::bit_util::BytesForBits(g)),
                                     hipMemcpyDeviceToHost, st));
    HIP_RETURN_NOT_OK(hipMemcpyAsync(&valid_count, d_counter, 8, hipMemcpyDeviceToHost, st));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    null_count = g - valid_count;
    if (!host_counts.empty()) ARROW_RETURN_NOT_OK(DecimalMeansInPlace(values->mutable_data(), host_counts.data(), g, s->options.min_count));
    if (s->options.skip_nulls) {
      if (null_count == 0) bitmap = nullptr;  // Finish allocates a bitmap only when a group is null
    } else {
      null_count = arrow::kUnknownNullCount;
    }
  }
  *out = arrow::Datum(ArrayData::Make(s->out_type != nullptr ? s->out_type : SumOutType(s->num_type), g,
                                      {std::move(bitmap), std::move(values)}, null_count));
  return Status::OK();
}

// The cast meta-function override.
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- cast between the numeric types
// Cast kernels live in a private table (GetCastFunction, cpp/src/arrow/compute/cast.cc:207-214)
// whose DispatchExact returns the FIRST exact-type match (cast.cc:170-205), so an added kernel
// would never be chosen.  The public route is the one the registry offers: re-register the
// "cast" MetaFunction (AddFunction(..., allow_overwrite=true), registry.h:69) with a wrapper that
// takes device-resident numeric arrays (and large host float64 -> float32 ones) and hands every other
// cast to the stock meta-function.
// Semantics: CastPrimitive<O, I>::Exec (scalar_cast_internal.cc:41-53) + the checks of scalar_cast_numeric.cc;
// validity shared or copied like NullHandling::INTERSECTION does for one input.
class RocmCastMetaFunction : public cp::MetaFunction {
 public:
  explicit RocmCastMetaFunction(std::shared_ptr<cp::Function> stock)
      : cp::MetaFunction("cast", cp::Arity::Unary(), stock->doc(), stock->default_options()),
        stock_(std::move(stock)) {}

  arrow::Result<arrow::Datum> ExecuteImpl(const std::vector<arrow::Datum>& args,
                                          const cp::FunctionOptions* options,
                                          cp::ExecContext* ctx) const override {
    const auto* cast_options = static_cast<const cp::CastOptions*>(options);
    // large float64 -> float32 HOST arrays are staged through HBM; every other host cast stays on the stock kernels
    if (cast_options != nullptr && cast_options->to_type.type != nullptr &&
        cast_options->to_type.id() == Type::FLOAT && args.size() == 1 && args[0].is_array() &&
        args[0].array()->type->id() == Type::DOUBLE && args[0].length() >= g_min_rows_streaming.load() &&
        IsHost(ArraySpan(*args[0].array()))) {
      return CastF64F32(*args[0].array(), ctx);
    }
    if (args.size() == 1 && args[0].is_array() && DataOnRocm(*args[0].array())) {
      if (cast_options != nullptr && cast_options->to_type.type != nullptr &&
          cast_options->to_type.type->Equals(*args[0].array()->type)) {
        return args[0];      // same type: zero-copy, as the reference does (cast.cc:108-112)
      }
      // every pair of the ten numeric types: CastNumberToNumberUnsafe + the reference's checks
      // (scalar_cast_numeric.cc:41-60, 62-207, 229-279) in arx_cast_numeric
      if (cast_options != nullptr && cast_options->to_type.type != nullptr) {
        const int from_num = NumTypeId(args[0].array()->type->id()), to_num = NumTypeId(cast_options->to_type.id());
        if (from_num >= 0 && to_num >= 0) return CastNumericDevice(*args[0].array(), from_num, to_num, *cast_options);
      }
      // (the stock kernels would read HBM addresses from the CPU)
      return Status::NotImplemented("arrow_amd: cast of a device-resident ", args[0].array()->type->ToString(), " array to ",
                                    cast_options != nullptr && cast_options->to_type.type != nullptr
                                        ? cast_options->to_type.type->ToString() : std::string("?"));
    }
    CountStock(kFnCast);
    return stock_->Execute(args, options, ctx);
  }

 private:
  static int NumTypeId(Type::type id) {
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

  // validity of a unary device kernel's output: the input's bitmap shared (offset 0) or re-based, exact null count
  static Status UnaryDeviceValidity(const ArrayData& in, const ArxSpan& sp, hipStream_t st, std::shared_ptr<Buffer>* validity,
                                    int64_t* null_count) {
    const int64_t n = in.length;
    *null_count = 0;
    if (sp.validity == nullptr || n == 0) return Status::OK();
    if (in.offset == 0) {
      *validity = in.buffers[0];
    } else {
      ARROW_ASSIGN_OR_RAISE(*validity, AllocDevice(((n + 63) / 64) * 8));
      ARROW_RETURN_NOT_OK(FromArx(arx_bitmap_copy(sp.validity, sp.offset, n, reinterpret_cast<void*>((*validity)->mutable_address()), st)));
    }
    *null_count = in.null_count.load();
    if (*null_count < 0 || in.offset != 0) {
      ARROW_ASSIGN_OR_RAISE(*null_count, DeviceNullCount(**validity, n, st));
    }
    return Status::OK();
  }

  static arrow::Result<arrow::Datum> CastNumericDevice(const ArrayData& in, int from_num, int to_num,
                                                       const cp::CastOptions& options) {
    static const int widths[10] = {1, 1, 2, 2, 4, 4, 8, 8, 4, 8};
    const int64_t n = in.length;
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    ARROW_ASSIGN_OR_RAISE(auto out_values, AllocDevice(std::max<int64_t>(n, 1) * widths[to_num]));
    ArxSpan sp{};
    ARROW_RETURN_NOT_OK(DeviceSpan(ArraySpan(in), &sp));
    void* ws = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(kFlag, 64, &ws));
    ARROW_RETURN_NOT_OK(FromArx(arx_cast_numeric(&sp, from_num, to_num, options.allow_int_overflow ? 1 : 0,
                                                 options.allow_float_truncate ? 1 : 0, ws, 64,
                                                 reinterpret_cast<void*>(out_values->mutable_address()), st)));
    std::shared_ptr<Buffer> validity;
    int64_t null_count = 0;
    ARROW_RETURN_NOT_OK(UnaryDeviceValidity(in, sp, st, &validity, &null_count));
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    CountGpu(kFnCast);
    return arrow::Datum(ArrayData::Make(options.to_type.GetSharedPtr(), n, {std::move(validity), std::move(out_values)}, null_count));
  }

  static arrow::Result<arrow::Datum> CastF64F32(const ArrayData& in, cp::ExecContext* ctx) {
    const int64_t n = in.length;
    hipStream_t st;
    ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
    void *din = nullptr, *dout = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(kValues, static_cast<size_t>(n) * 8 + 16, &din));
    ARROW_RETURN_NOT_OK(t_scratch.Get(kOutData, static_cast<size_t>(n) * 4 + 16, &dout));
    ARROW_ASSIGN_OR_RAISE(std::shared_ptr<Buffer> out_values,
                          arrow::AllocateBuffer(n * 4, ctx->memory_pool()));
    HIP_RETURN_NOT_OK(hipMemcpyAsync(din, in.GetValues<double>(1), static_cast<size_t>(n) * 8,
                                     hipMemcpyHostToDevice, st));
    const ArxSpan staged{nullptr, din, 0, n, 0};   // (every slot is converted; validity stays on the host)
    ARROW_RETURN_NOT_OK(FromArx(arx_cast_numeric(&staged, ARX_NUM_FLOAT64, ARX_NUM_FLOAT32, 0, 0, nullptr, 0, dout, st)));
    HIP_RETURN_NOT_OK(hipMemcpyAsync(out_values->mutable_data(), dout, static_cast<size_t>(n) * 4,
                                     hipMemcpyDeviceToHost, st));
    std::shared_ptr<Buffer> validity;
    if (in.null_count != 0 && in.buffers[0] != nullptr) {
      if (in.offset == 0) {
        validity = in.buffers[0];  // zero-copy, as PropagateNulls does (exec.cc:1222-1281)
      } else {
        ARROW_ASSIGN_OR_RAISE(validity, arrow::internal::CopyBitmap(ctx->memory_pool(),
                                                                    in.buffers[0]->data(),
                                                                    in.offset, n));
      }
    }
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    CountGpu(kFnCast);
    const int64_t null_count = validity ? in.null_count.load() : 0;
    return arrow::Datum(ArrayData::Make(arrow::float32(), n, {std::move(validity), std::move(out_values)},
                                        null_count));
  }

  std::shared_ptr<cp::Function> stock_;
};

// What every NO_PREALLOCATE kernel twin shares: its registration, the record of the reference's kernel, its init, its host
// fallback, and the device result of the functions whose rows are sub-ranges of the input's.
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- kernel twins
// A scalar function taken over is registered as a twin: a copy of the reference's kernel with NullHandling::
// COMPUTED_NO_PREALLOCATE + MemAllocation::NO_PREALLOCATE (the ScalarExecutor's own preallocation and null propagation,
// exec.cc, run on the CPU and cannot touch device buffers).  Its exec runs the device kernel for device-resident
// operands; for host operands it calls RunStockPrepared / RunStockVarLength below on the stock exec its TwinData
// remembers.  AppendTwins registers it, InstallTwin fills it in.

// A value type of a twin (or of array_filter / array_take / array_sort_indices): the concrete type used to find the
// stock kernel and the matcher the added kernel is registered under (parametric types match by type id).
struct ValueType {
  std::shared_ptr<arrow::DataType> probe;
  cp::InputType match;
  ValueType(std::shared_ptr<arrow::DataType> t) : probe(t), match(t) {}  // NOLINT
  ValueType(std::shared_ptr<arrow::DataType> t, Type::type id) : probe(std::move(t)), match(id) {}
  ValueType(std::shared_ptr<arrow::DataType> t, cp::InputType m) : probe(std::move(t)), match(std::move(m)) {}
};

// boolean and the fixed-width types coalesce and if_else take on the device.  The one rule for parametric types (unit,
// time zone, precision / scale): they match by type id.
std::vector<ValueType> FixedWidthTwinTypes(bool with_decimal128) {
  std::vector<std::shared_ptr<arrow::DataType>> types = {
      arrow::boolean(), arrow::int8(), arrow::uint8(), arrow::int16(), arrow::uint16(), arrow::int32(), arrow::uint32(), arrow::int64(),
      arrow::uint64(), arrow::float32(), arrow::float64(), arrow::date32(), arrow::date64(), arrow::time32(arrow::TimeUnit::SECOND),
      arrow::time64(arrow::TimeUnit::MICRO), arrow::timestamp(arrow::TimeUnit::SECOND), arrow::duration(arrow::TimeUnit::SECOND)};
  if (with_decimal128) types.push_back(arrow::decimal128(38, 9));
  std::vector<ValueType> out;
  for (const auto& t : types) {
    const bool parametric = arrow::is_temporal(t->id()) || t->id() == Type::DURATION || t->id() == Type::DECIMAL128;
    out.push_back(parametric ? ValueType(t, t->id()) : ValueType(t));
  }
  return out;
}

// Says what a twin installs over the copy of the reference's kernel it is handed (which still holds the stock exec, init
// and data): most families call InstallTwin below.  false: this type gets no twin.
using TwinInstall = std::function<arrow::Result<bool>(const ValueType&, cp::ScalarKernel*)>;

// Append one twin per type to the scalar function `name`: the reference's kernel is found by DispatchExact on probe(type)
// — a type it does not take is an error unless skip_undispatched — copied, handed to `install`, given the two
// NO_PREALLOCATE enums and added after the reference's own kernels (dispatch takes the last match).
Status AppendTwins(cp::FunctionRegistry* reg, const std::string& name, const std::vector<ValueType>& types,
                   const std::function<std::vector<arrow::TypeHolder>(const std::shared_ptr<arrow::DataType>&)>& probe,
                   const TwinInstall& install, bool skip_undispatched = false) {
  ARROW_ASSIGN_OR_RAISE(auto fn, reg->GetFunction(name));
  if (fn->kind() != cp::Function::SCALAR) return Status::Invalid(name, " is not a scalar function");
  auto* sfn = static_cast<cp::ScalarFunction*>(fn.get());
  for (const ValueType& vt : types) {
    auto k0 = sfn->DispatchExact(probe(vt.probe));
    if (!k0.ok() && skip_undispatched) continue;
    ARROW_RETURN_NOT_OK(k0.status());
    cp::ScalarKernel twin = *static_cast<const cp::ScalarKernel*>(*k0);
    ARROW_ASSIGN_OR_RAISE(const bool add, install(vt, &twin));
    if (!add) continue;
    twin.null_handling = cp::NullHandling::COMPUTED_NO_PREALLOCATE;
    twin.mem_allocation = cp::MemAllocation::NO_PREALLOCATE;
    ARROW_RETURN_NOT_OK(sfn->AddKernel(std::move(twin)));
  }
  return Status::OK();
}

// What the executor prepares for the reference's kernel, read off the kernel's own enums.
struct StockContract {
  cp::NullHandling::type null_handling = cp::NullHandling::INTERSECTION;
  cp::MemAllocation::type mem_allocation = cp::MemAllocation::NO_PREALLOCATE;
};

// What a twin remembers of the reference's kernel it replaces, kept as the twin's Kernel::data.  A family that needs
// more derives from it (a table row, an op code).
struct TwinData : public cp::KernelState {
  Fn fn = kFnFilter;
  cp::ArrayKernelExec stock_exec = nullptr;
  cp::KernelInit stock_init;   // empty: the reference's kernel has no state
  StockContract contract;
};

// the record of a twin's kernel; null when the kernel carries none, another family's, or one without a stock exec
template <class Data = TwinData>
const Data* TwinDataOf(const cp::Kernel* k) {
  const Data* data = k != nullptr ? dynamic_cast<const Data*>(k->data.get()) : nullptr;
  return data != nullptr && data->stock_exec != nullptr ? data : nullptr;
}
Status TwinWithoutData() { return Status::Invalid("arrow_amd: a kernel twin ran without its data"); }

// What every install does with the copy AppendTwins hands it: check that the reference's kernel carries no data and is
// of the shape the family expects, remember its exec / init / contract in `data`, and install the twin's own signature
// ({vt.match} -> the reference's out type unless one is given), init (when the reference has one) and exec.
Status InstallTwin(const char* name, const ValueType& vt, cp::ScalarKernel* twin, bool shape_ok, std::shared_ptr<TwinData> data, Fn fn,
                   cp::KernelInit init, cp::ArrayKernelExec exec, std::shared_ptr<cp::KernelSignature> signature = nullptr) {
  if (twin->data != nullptr || !shape_ok) {
    return Status::Invalid("arrow_amd: the reference's ", name, " kernel of ", vt.probe->ToString(), " is not of the expected shape");
  }
  data->fn = fn;
  data->stock_exec = twin->exec;
  data->stock_init = twin->init;
  data->contract.null_handling = twin->null_handling;
  data->contract.mem_allocation = twin->mem_allocation;
  twin->data = std::move(data);
  twin->signature = signature != nullptr ? std::move(signature) : cp::KernelSignature::Make({vt.match}, twin->signature->out_type());
  if (twin->init && init) twin->init = std::move(init);
  twin->exec = exec;
  twin->can_write_into_slices = false;
  return Status::OK();
}

// The init of a twin whose reference kernel has one: the reference's init runs first (its state serves host batches and
// its option checks stay its own), then the options are copied for the device call.  kRequired: a call without options
// is the Invalid below; otherwise the copy keeps Options' defaults, as it does for options of another class (a
// function without options of its own is handed whatever the caller passed).  State: ShimState<Options> or a family's
// extension of it.
template <class Options, bool kRequired = false, class State = ShimState<Options>>
arrow::Result<std::unique_ptr<cp::KernelState>> TwinInit(cp::KernelContext* ctx, const cp::KernelInitArgs& args) {
  const TwinData* data = TwinDataOf(args.kernel);
  if (data == nullptr || !data->stock_init) return Status::Invalid("arrow_amd: a kernel twin was initialised without its data");
  auto state = std::make_unique<State>();
  ARROW_ASSIGN_OR_RAISE(state->stock, data->stock_init(ctx, args));
  if (kRequired && args.options == nullptr) return Status::Invalid("arrow_amd: ", kFnNames[data->fn], " without ", Options::kTypeName);
  if (args.options != nullptr && std::strcmp(args.options->type_name(), Options::kTypeName) == 0) {
    state->options = *static_cast<const Options*>(args.options);
  }
  return state;
}

// The output validity the executor would have prepared for the reference's kernel.
enum class TwinValidity {
  kNone,          // OUTPUT_NOT_NULL: no bitmap, null count 0
  kAllocate,      // COMPUTED_PREALLOCATE: a zeroed bitmap for the kernel to fill, null count unknown
  kIntersection,  // INTERSECTION (NullPropagator, exec.cc): no buffer when nothing can be null, a copy of the one bitmap
                  // that can hold nulls, BitmapAnd of two, all clear with null count n for a null scalar
};

// What the ScalarExecutor would have preallocated for the reference's kernel: `tmp` is an ArraySpan at offset 0 over
// the two buffers; null_count is the span's as prepared (0, n, an input's own or kUnknownNullCount).
struct PreparedOutput {
  std::shared_ptr<Buffer> validity, data;
  int64_t null_count = 0;
  cp::ExecResult tmp;

  // `validity` and `null_count` as the policy prepares them
  Status PrepareValidity(cp::KernelContext* ctx, const cp::ExecSpan& batch, TwinValidity policy) {
    const int64_t n = batch.length;
    if (policy == TwinValidity::kAllocate) {
      ARROW_ASSIGN_OR_RAISE(validity, ctx->AllocateBitmap(n));
      null_count = arrow::kUnknownNullCount;
    } else if (policy == TwinValidity::kIntersection) {
      bool null_scalar = false;
      const ArraySpan* with_nulls[2];
      int nv = 0;
      for (const cp::ExecValue& v : batch.values) {
        if (v.is_scalar()) {
          null_scalar = null_scalar || !v.scalar->is_valid;
        } else if (v.array.MayHaveNulls()) {
          if (nv == 2) return Status::NotImplemented("arrow_amd: the validity intersection of more than two arrays");
          with_nulls[nv++] = &v.array;
        }
      }
      if (null_scalar) {
        ARROW_ASSIGN_OR_RAISE(validity, ctx->AllocateBitmap(n));
        null_count = n;
      } else if (nv == 1) {
        ARROW_ASSIGN_OR_RAISE(validity, arrow::internal::CopyBitmap(ctx->memory_pool(), with_nulls[0]->buffers[0].data,
                                                                    with_nulls[0]->offset, n));
        null_count = with_nulls[0]->null_count;
      } else if (nv == 2) {
        ARROW_ASSIGN_OR_RAISE(validity, arrow::internal::BitmapAnd(ctx->memory_pool(), with_nulls[0]->buffers[0].data,
                                                                   with_nulls[0]->offset, with_nulls[1]->buffers[0].data,
                                                                   with_nulls[1]->offset, n, 0));
        null_count = arrow::kUnknownNullCount;
      }
    }
    return Status::OK();
  }

  // width: bytes per value, 0 for a bitmap of batch.length bits
  Status Prepare(cp::KernelContext* ctx, const cp::ExecSpan& batch, const arrow::DataType* type, int width, TwinValidity policy) {
    const int64_t n = batch.length;
    if (width == 0) {
      ARROW_ASSIGN_OR_RAISE(data, ctx->AllocateBitmap(n));
    } else {
      ARROW_ASSIGN_OR_RAISE(data, ctx->Allocate(n * width));
    }
    ARROW_RETURN_NOT_OK(PrepareValidity(ctx, batch, policy));
    ArraySpan span;
    span.type = type;
    span.length = n;
    span.offset = 0;
    span.null_count = null_count;
    if (validity) {
      span.buffers[0].data = validity->mutable_data();
      span.buffers[0].size = validity->size();
    }
    span.buffers[1].data = data->mutable_data();
    span.buffers[1].size = data->size();
    tmp.value = std::move(span);
    return Status::OK();
  }

  // the filled buffers become `out`'s; the null count it reports is the prepared one
  void MoveInto(ArrayData* out) {
    out->buffers.resize(2);
    out->buffers[0] = std::move(validity);
    out->buffers[1] = std::move(data);
    out->null_count = null_count;
  }
};

// The host half of a twin: prepare the output, run the reference's exec (with its own KernelState installed, when
// one is given) and hand the buffers to `out`.  stock_null_count, when asked for: what the exec left in the span.
Status RunStockPrepared(Fn fn, cp::ArrayKernelExec exec, std::optional<cp::KernelState*> stock_state, int width,
                        TwinValidity policy, cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out,
                        int64_t* stock_null_count = nullptr) {
  ArrayData* out_arr = out->array_data().get();
  PreparedOutput p;
  ARROW_RETURN_NOT_OK(p.Prepare(ctx, batch, out_arr->type.get(), width, policy));
  ARROW_RETURN_NOT_OK(RunStock(fn, exec, stock_state, ctx, batch, &p.tmp));
  if (stock_null_count != nullptr) *stock_null_count = p.tmp.array_span()->null_count;
  p.MoveInto(out_arr);
  return Status::OK();
}

// The host half of a twin whose result is a variable-length column (utf8 / binary and their large forms).  Such a
// reference kernel writes into the ArrayData itself; what the executor prepares for it is read off the kernel's own
// enums (the StockContract its TwinData remembers): the validity as its null_handling says, and, when its
// mem_allocation is PREALLOCATE, the offsets buffer (batch.length + 1 entries; the executor preallocates no data buffer
// for a variable-length type).  Whatever is not prepared the exec allocates.
Status RunStockVarLength(Fn fn, cp::ArrayKernelExec exec, std::optional<cp::KernelState*> stock_state, StockContract contract,
                         cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  ArrayData* out_arr = out->array_data().get();
  const TwinValidity policy = contract.null_handling == cp::NullHandling::INTERSECTION           ? TwinValidity::kIntersection
                              : contract.null_handling == cp::NullHandling::COMPUTED_PREALLOCATE ? TwinValidity::kAllocate
                                                                                                 : TwinValidity::kNone;
  PreparedOutput p;
  ARROW_RETURN_NOT_OK(p.PrepareValidity(ctx, batch, policy));
  out_arr->length = batch.length;
  out_arr->offset = 0;
  out_arr->buffers.assign(3, nullptr);
  out_arr->buffers[0] = std::move(p.validity);
  out_arr->null_count = p.null_count;
  if (contract.mem_allocation == cp::MemAllocation::PREALLOCATE) {
    ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], ctx->Allocate((batch.length + 1) * BinaryOffsetWidth(out_arr->type->id())));
  }
  return RunStock(fn, exec, stock_state, ctx, batch, out);
}

// The bytes of a valid scalar operand of a device call: one byte 0 / 1 for a boolean (width 0), the value of a
// fixed-width scalar otherwise.  Returns the scalar's width; nothing is written when that is not `width`.
int64_t FixedWidthScalarBytes(const arrow::Scalar& sc, int width, void* out) {
  if (width == 0) {
    *static_cast<uint8_t*>(out) = static_cast<const arrow::BooleanScalar&>(sc).value ? 1 : 0;
    return 0;
  }
  const auto bytes = static_cast<const arrow::internal::PrimitiveScalarBase&>(sc).view();
  if (static_cast<int>(bytes.size()) == width) std::memcpy(out, bytes.data(), bytes.size());
  return static_cast<int64_t>(bytes.size());
}

// The input's validity at offset 0 into out_arr->buffers[0] (none when it has no nulls) and its null count.
Status CopyInputValidity(const ArxBinarySpan& vs, int64_t n, hipStream_t st, ArrayData* out_arr) {
  out_arr->null_count = 0;
  if (vs.validity == nullptr || vs.null_count == 0) return Status::OK();
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

// The device result of a function that makes one variable-length row from each row of the input (slices, trims,
// replace_substring): `offsets_call` (vs, offset_width, ws, ws_bytes, d_off, &total, st) writes the n + 1 offsets and
// leaves in the workspace of ws_bytes bytes what `data_call` (vs, offset_width, ws, ws_bytes, d_off, total, d_data, st)
// needs to write the bytes; the validity is the input's.  One synchronisation, at the end.
template <class OffsetsCall, class DataCall>
Status VarLengthResultOnDevice(Fn fn, const ArxBinarySpan& vs, int offset_width, hipStream_t st, size_t ws_bytes, OffsetsCall&& offsets_call,
                               DataCall&& data_call, ArrayData* out_arr) {
  const int64_t n = vs.length;
  out_arr->length = n;
  out_arr->offset = 0;
  out_arr->buffers.assign(3, nullptr);
  ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice((n + 1) * offset_width));
  void* ws = nullptr;
  ARROW_RETURN_NOT_OK(t_scratch.Get(kBinWs, ws_bytes, &ws));
  void* d_off = reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address());
  int64_t total = 0;
  ARROW_RETURN_NOT_OK(FromArx(offsets_call(&vs, offset_width, ws, ws_bytes, d_off, &total, st)));
  ARROW_ASSIGN_OR_RAISE(out_arr->buffers[2], AllocDevice(std::max<int64_t>(total, 8)));
  ARROW_RETURN_NOT_OK(FromArx(data_call(&vs, offset_width, ws, ws_bytes, d_off, total,
                                        reinterpret_cast<void*>(out_arr->buffers[2]->mutable_address()), st)));
  ARROW_RETURN_NOT_OK(CopyInputValidity(vs, n, st, out_arr));
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (this thread's scratch may be released after return)
  CountGpu(fn);
  return Status::OK();
}

// The same for a function whose every row is a sub-range of the input's row (slices, trims): the offsets call leaves each
// row's source position in the workspace and arx_string_slice_data copies the bytes.
template <class OffsetsCall>
Status SubRangeResultOnDevice(Fn fn, const ArxBinarySpan& vs, int offset_width, hipStream_t st, OffsetsCall&& offsets_call,
                              ArrayData* out_arr) {
  return VarLengthResultOnDevice(fn, vs, offset_width, st, arx_string_slice_workspace_bytes(vs.length, offset_width),
                                 std::forward<OffsetsCall>(offsets_call), arx_string_slice_data, out_arr);
}

// is_in / index_in on device-resident arrays (csrc/set_lookup.hip).
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- set lookup
// The reference's kernels (kernels/scalar_set_lookup.cc) build a memo table of SetLookupOptions::value_set in their
// init and probe it per batch.  The added kernels keep that init — every type has its own; the one of the call's input
// type is found among the reference's kernels — so its state serves host batches and its type checks raise the
// reference's errors.  The device table is built from the same value set on the first device-resident batch (an init
// cannot know where the batches will live), once per kernel state: an Acero filter reuses it for every batch.  Type resolution as the reference's: the value set is cast to
// the input's type on the host when that cast is safe, otherwise the input is cast to the value set's type on the device
// (the registered casts; a pair without one is refused with a Status).  Outputs stay in HBM: is_in a bitmap without
// nulls, index_in int32 indices with the bitmap of hits as validity.  Host batches run the reference's exec on the
// outputs the executor would have preallocated for it (COMPUTED_PREALLOCATE: a validity bitmap and the values).
struct SetLookupKernelData : public TwinData {
  bool index = false;
};
// the reference's kernels of is_in [0] / index_in [1] as registered before the shim's.  Unlike the other twins these do
// not run the stock exec / init their TwinData remembers (the probe type's): an added kernel matches a whole type id
// (every timestamp unit, every decimal128 precision) while the reference's init differs per concrete type, so the init
// and exec of a call are those of the reference's kernel that matches its concrete input type, searched per call
std::vector<cp::ScalarKernel> g_stock_set_lookup[2];

struct DeviceSetLookupState : public cp::KernelState {
  std::unique_ptr<cp::KernelState> stock;
  cp::ArrayKernelExec stock_exec = nullptr;
  cp::SetLookupOptions options;
  std::shared_ptr<arrow::DataType> input_type;
  std::mutex mu;
  bool built = false;
  std::shared_ptr<arrow::DataType> compare_type;   // the type rows are compared in
  bool cast_input = false;
  std::shared_ptr<ArrayData> set;                  // the value set on the device, in compare_type
  std::shared_ptr<Buffer> table_buf;
  void* table = nullptr;
  int key_width = 0;                               // 1 .. 16 fixed widths, 0 boolean, -1 binary
  int set_offset_width = 4;
};

// key width of a type on the device table: 1 .. 16 by bits, 0 boolean, -1 binary (offset width 4 / 8); -2 = none
int SetLookupKeyWidth(const arrow::DataType& t, int* offset_width) {
  *offset_width = BinaryOffsetWidth(t.id());
  switch (t.id()) {
    case Type::BOOL: return 0;
    case Type::STRING: case Type::BINARY: case Type::LARGE_STRING: case Type::LARGE_BINARY: return -1;
    case Type::DECIMAL128: return 16;
    case Type::INT8: case Type::UINT8: case Type::INT16: case Type::UINT16: case Type::INT32: case Type::UINT32:
    case Type::INT64: case Type::UINT64: case Type::FLOAT: case Type::DOUBLE: case Type::DATE32: case Type::DATE64:
    case Type::TIME32: case Type::TIME64: case Type::TIMESTAMP: case Type::DURATION:
      return FixedByteWidth(t);
    default: return -2;
  }
}

arrow::Result<std::unique_ptr<cp::KernelState>> SetLookupInit(cp::KernelContext* ctx, const cp::KernelInitArgs& args) {
  const auto* data = TwinDataOf<SetLookupKernelData>(args.kernel);
  if (data == nullptr || args.options == nullptr) return Status::Invalid("arrow_amd: set lookup kernel without its data or options");
  auto state = std::make_unique<DeviceSetLookupState>();
  state->options = *static_cast<const cp::SetLookupOptions*>(args.options);
  state->input_type = args.inputs[0].GetSharedPtr();
  const cp::ScalarKernel* stock = nullptr;
  for (const cp::ScalarKernel& k : g_stock_set_lookup[data->index ? 1 : 0]) {
    if (k.signature->MatchesInputs(args.inputs)) stock = &k;   // (the last match, as DispatchExact picks)
  }
  if (stock == nullptr || !stock->init) return Status::Invalid("arrow_amd: no reference set lookup kernel for ", state->input_type->ToString());
  state->stock_exec = stock->exec;
  ARROW_ASSIGN_OR_RAISE(state->stock, stock->init(ctx, args));   // the reference's table and its type checks
  return state;
}

Status SetLookupBuild(DeviceSetLookupState* s, cp::ExecContext* exec_ctx, hipStream_t st) {
  const arrow::Datum& vs = s->options.value_set;
  std::shared_ptr<arrow::Array> set;
  if (vs.is_array()) {
    set = vs.make_array();
  } else if (vs.is_chunked_array()) {            // indexed across its chunks
    const auto& chunks = vs.chunked_array()->chunks();
    if (chunks.empty()) {
      ARROW_ASSIGN_OR_RAISE(set, arrow::MakeEmptyArray(vs.type()));
    } else {
      ARROW_ASSIGN_OR_RAISE(set, arrow::Concatenate(chunks));
    }
  } else {
    return Status::Invalid("arrow_amd: is_in / index_in value_set must be an array or chunked array");
  }
  if (DataTouchesRocm(*set->data())) return Status::NotImplemented("arrow_amd: a device-resident value_set for is_in / index_in");
  s->compare_type = s->input_type;
  if (!set->type()->Equals(*s->input_type)) {
    auto cast = cp::Cast(*set, s->input_type, cp::CastOptions::Safe(), exec_ctx);
    if (cast.ok()) {
      set = *cast;
    } else {
      s->compare_type = set->type();
      s->cast_input = true;
    }
  }
  s->key_width = SetLookupKeyWidth(*s->compare_type, &s->set_offset_width);
  if (s->key_width == -2) {
    return Status::NotImplemented("arrow_amd: is_in / index_in in ", s->compare_type->ToString(), " on device-resident arrays");
  }
  ARROW_ASSIGN_OR_RAISE(auto mm, RocmMemoryManagerFor(0));
  auto dev = set->data()->Copy();
  for (auto& b : dev->buffers) {
    if (b != nullptr) {
      ARROW_ASSIGN_OR_RAISE(b, arrow::MemoryManager::CopyBuffer(b, mm));
    }
  }
  s->set = dev;
  const int64_t m = dev->length;
  ARROW_ASSIGN_OR_RAISE(auto table, AllocAligned(static_cast<int64_t>(arx_set_lookup_state_bytes(m, s->key_width))));
  s->table_buf = std::move(table.buffer);
  s->table = table.ptr;
  const ArraySpan span(*dev);
  if (s->key_width == -1) {
    ArxBinarySpan bs{};
    ARROW_RETURN_NOT_OK(DeviceBinarySpan(span, &bs));
    bs.null_count = set->null_count();
    ARROW_RETURN_NOT_OK(FromArx(arx_set_lookup_build_binary(s->table, &bs, s->set_offset_width, 64, st)));
  } else {
    ArxSpan sp{};
    ARROW_RETURN_NOT_OK(DeviceSpan(span, &sp));
    sp.null_count = set->null_count();
    ARROW_RETURN_NOT_OK(FromArx(arx_set_lookup_build(s->table, &sp, s->key_width, st)));
  }
  s->built = true;
  return Status::OK();
}

// a host batch: the reference's exec on what the executor preallocates for its COMPUTED_PREALLOCATE kernels
Status SetLookupStock(cp::KernelContext* ctx, const SetLookupKernelData& kd, DeviceSetLookupState* s, const cp::ExecSpan& batch,
                      cp::ExecResult* out) {
  int64_t nulls = 0;
  ARROW_RETURN_NOT_OK(RunStockPrepared(kd.fn, s->stock_exec, s->stock.get(), kd.index ? 4 : 0,
                                       TwinValidity::kAllocate, ctx, batch, out, &nulls));
  ArrayData* out_arr = out->array_data().get();
  if (nulls < 0) nulls = batch.length - arrow::internal::CountSetBits(out_arr->buffers[0]->data(), 0, batch.length);
  out_arr->null_count = nulls;
  return Status::OK();
}

Status SetLookupExec(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  const auto* kd = TwinDataOf<SetLookupKernelData>(ctx->kernel());
  auto* s = static_cast<DeviceSetLookupState*>(ctx->state());
  if (kd == nullptr || s == nullptr) return Status::Invalid("arrow_amd: set lookup kernel ran without its data or state");
  if (!batch[0].is_array() || !SpanTouchesRocm(batch[0].array)) return SetLookupStock(ctx, *kd, s, batch, out);
  const char* fname = kd->index ? "index_in" : "is_in";
  const auto behaviour = s->options.GetNullMatchingBehavior();
  if (behaviour != cp::SetLookupOptions::MATCH && behaviour != cp::SetLookupOptions::SKIP) {
    return Status::NotImplemented("arrow_amd: ", fname, " with null_matching_behavior EMIT_NULL / INCONCLUSIVE on device-resident arrays");
  }
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  {
    std::lock_guard<std::mutex> lock(s->mu);
    if (!s->built) ARROW_RETURN_NOT_OK(SetLookupBuild(s, ctx->exec_context(), st));
  }
  // the rows in the compared type: as they are, or cast on the device
  std::shared_ptr<ArrayData> cast_rows;
  ArraySpan rows = batch[0].array;
  if (s->cast_input) {
    ARROW_ASSIGN_OR_RAISE(arrow::Datum c, cp::Cast(arrow::Datum(batch[0].array.ToArrayData()), s->compare_type,
                                                 cp::CastOptions::Safe(), ctx->exec_context()));
    cast_rows = c.array();
    rows = ArraySpan(*cast_rows);
  }
  const int64_t n = rows.length;
  const int64_t m = s->set->length;
  ArrayData* out_arr = out->array_data().get();
  out_arr->buffers.assign(2, nullptr);
  ARROW_ASSIGN_OR_RAISE(auto bits, AllocDevice(BitmapBytes(n)));
  std::shared_ptr<Buffer> idx;
  if (kd->index) {
    ARROW_ASSIGN_OR_RAISE(idx, AllocDevice(std::max<int64_t>(n, 1) * 4));
  }
  void* d_bits = reinterpret_cast<void*>(bits->mutable_address());
  int32_t* d_idx = kd->index ? reinterpret_cast<int32_t*>(idx->mutable_address()) : nullptr;
  const int skip = behaviour == cp::SetLookupOptions::SKIP ? 1 : 0;
  if (s->key_width == -1) {
    int offset_width = 4;
    SetLookupKeyWidth(*rows.type, &offset_width);
    ArxBinarySpan vs{}, set{};
    ARROW_RETURN_NOT_OK(DeviceBinarySpan(rows, &vs));
    ARROW_RETURN_NOT_OK(DeviceBinarySpan(ArraySpan(*s->set), &set));
    ARROW_RETURN_NOT_OK(FromArx(kd->index ? arx_set_lookup_index_in_binary(s->table, &set, s->set_offset_width, 64, &vs, offset_width,
                                                                           skip, d_idx, d_bits, st)
                                          : arx_set_lookup_is_in_binary(s->table, &set, s->set_offset_width, 64, &vs, offset_width, skip,
                                                                        d_bits, st)));
  } else {
    ArxSpan sp{};
    ARROW_RETURN_NOT_OK(DeviceSpan(rows, &sp));
    ARROW_RETURN_NOT_OK(FromArx(kd->index ? arx_set_lookup_index_in(s->table, m, s->key_width, &sp, skip, d_idx, d_bits, st)
                                          : arx_set_lookup_is_in(s->table, m, s->key_width, &sp, skip, d_bits, st)));
  }
  if (kd->index) {
    out_arr->buffers[0] = bits;
    out_arr->buffers[1] = idx;
    ARROW_ASSIGN_OR_RAISE(out_arr->null_count, DeviceNullCount(*bits, n, st));
  } else {
    out_arr->buffers[1] = bits;
    out_arr->null_count = 0;
  }
  HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (the cast rows and this thread's scratch may be released after return)
  CountGpu(kd->fn);
  return Status::OK();
}

// the added kernels: one per type of the device path, matched by type id, appended after the reference's (dispatch takes
// the last match); every other type keeps the reference's kernel behind the device guard (plugin/device_guard.inc)
Status RegisterSetLookup(cp::FunctionRegistry* reg, const char* name, bool index) {
  ARROW_ASSIGN_OR_RAISE(auto fn, reg->GetFunction(name));
  if (fn->kind() != cp::Function::SCALAR) return Status::Invalid(name, " is not a scalar function");
  auto& stock = g_stock_set_lookup[index ? 1 : 0];
  stock.clear();
  for (const cp::ScalarKernel* k : static_cast<cp::ScalarFunction*>(fn.get())->kernels()) stock.push_back(*k);
  const std::vector<ValueType> types = {
      arrow::boolean(), arrow::int8(), arrow::uint8(), arrow::int16(), arrow::uint16(), arrow::int32(), arrow::uint32(),
      arrow::int64(), arrow::uint64(), arrow::float32(), arrow::float64(), arrow::date32(), arrow::date64(),
      {arrow::time32(arrow::TimeUnit::SECOND), Type::TIME32}, {arrow::time64(arrow::TimeUnit::NANO), Type::TIME64},
      {arrow::timestamp(arrow::TimeUnit::NANO), Type::TIMESTAMP}, {arrow::duration(arrow::TimeUnit::NANO), Type::DURATION},
      {arrow::decimal128(38, 9), Type::DECIMAL128}, arrow::utf8(), arrow::binary(), arrow::large_utf8(), arrow::large_binary()};
  return AppendTwins(reg, name, types, [](const auto& t) { return std::vector<arrow::TypeHolder>{t}; },
                     [name, index](const ValueType& vt, cp::ScalarKernel* twin) -> arrow::Result<bool> {
                       if (twin->data != nullptr || !twin->init) return false;   // (none of the reference's set lookup kernels carries data)
                       auto data = std::make_shared<SetLookupKernelData>();
                       data->index = index;
                       ARROW_RETURN_NOT_OK(InstallTwin(name, vt, twin, true, std::move(data), index ? kFnIndexIn : kFnIsIn, SetLookupInit, SetLookupExec));
                       return true;
                     },
                     /*skip_undispatched=*/true);   // a type the reference does not look up either
}

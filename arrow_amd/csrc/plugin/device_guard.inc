// Guards on the reference's own kernels of the functions this shim extends.
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- device arrays must not reach a CPU kernel
// Arrow's executors hand any kernel whatever buffers the arrays hold: a stock CPU kernel given a kROCM array reads
// Buffer::data() == nullptr (buffer.h:221-226) or an HBM address — a crash inside libarrow.  The shim registers device
// kernels for the types of its path; for every OTHER type of the functions it touches (fixed_size_binary under `equal`, booleans
// under `unique`, decimals under `add`, large_utf8 under `array_filter`, ...) the reference kernel is re-registered as a
// copy whose exec first looks at the operands: device-resident -> NotImplemented naming the function and the type,
// host -> the reference's exec, untouched (same init, same null handling, same preallocation contract: the copy keeps
// every field of the stock kernel).  Dispatch takes the LAST matching kernel (function.cc:123-157), so after the guards
// the shim's own kernels are appended once more.  The original exec travels in Kernel::data, which the executors make
// reachable through KernelContext::kernel() (function.cc:219, expression.cc:588,783); stock kernels that use `data`
// themselves run behind a copy of themselves installed as ctx->kernel() (round 4) — except those of `less` / `less_equal`, which the reference builds as flipped copies
// of the `greater` / `greater_equal` kernels, same order, the unflipped exec in `data` (MakeFlippedFunction /
// FlippedCompare, scalar_compare.cc:436-445): their guards swap the operands and call that exec themselves.
struct GuardData : public cp::KernelState {
  cp::ArrayKernelExec exec = nullptr;
  cp::VectorKernel::ChunkedExec exec_chunked = nullptr;
  bool flipped = false;
  std::string function;
  // a stock kernel that reads its own Kernel::data (the comparisons' CompareData, ...): a copy of it, data included, is what
  // the reference exec sees as ctx->kernel() while it runs (KernelContext::SetKernel) — ADVICE r3: such kernels used to be
  // left unguarded
  std::shared_ptr<cp::Kernel> original;
};

const GuardData* GuardOf(cp::KernelContext* ctx) {
  return ctx->kernel() != nullptr ? dynamic_cast<const GuardData*>(ctx->kernel()->data.get()) : nullptr;
}

Status RefuseDevice(const GuardData& g, const arrow::DataType& type) {
  return Status::NotImplemented("arrow_amd: ", g.function, " of ", type.ToString(), " on device-resident arrays: no device "
                                "kernel is registered for this type, and the reference's CPU kernel cannot read device memory");
}

Status GuardedExec(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  const GuardData* g = GuardOf(ctx);
  if (g == nullptr || g->exec == nullptr) return Status::Invalid("arrow_amd: a guarded kernel ran without its kernel backreference");
  for (const cp::ExecValue& v : batch.values) {
    if (v.is_array() && SpanTouchesRocm(v.array)) return RefuseDevice(*g, *v.array.type);
  }
  if (g->flipped && batch.values.size() == 2) {
    cp::ExecSpan flipped_batch = batch;
    std::swap(flipped_batch.values[0], flipped_batch.values[1]);
    return g->exec(ctx, flipped_batch, out);
  }
  if (g->original != nullptr) {
    const cp::Kernel* mine = ctx->kernel();
    ctx->SetKernel(g->original.get());
    const Status st = g->exec(ctx, batch, out);
    ctx->SetKernel(mine);
    return st;
  }
  return g->exec(ctx, batch, out);
}

Status GuardedExecChunked(cp::KernelContext* ctx, const cp::ExecBatch& batch, arrow::Datum* out) {
  const GuardData* g = GuardOf(ctx);
  if (g == nullptr || g->exec_chunked == nullptr) return Status::Invalid("arrow_amd: a guarded kernel ran without its kernel backreference");
  for (const arrow::Datum& v : batch.values) {
    if (v.is_array() && DataTouchesRocm(*v.array())) return RefuseDevice(*g, *v.type());
    if (v.is_chunked_array()) {
      for (const auto& chunk : v.chunked_array()->chunks()) {
        if (DataTouchesRocm(*chunk->data())) return RefuseDevice(*g, *v.type());
      }
    }
  }
  if (g->original != nullptr) {
    const cp::Kernel* mine = ctx->kernel();
    ctx->SetKernel(g->original.get());
    const Status st = g->exec_chunked(ctx, batch, out);
    ctx->SetKernel(mine);
    return st;
  }
  return g->exec_chunked(ctx, batch, out);
}

// unflipped: for `less` / `less_equal`, the stock kernels of `greater` / `greater_equal` in registration order (else empty)
template <typename FunctionT, typename KernelT>
Status GuardKernels(cp::Function* fn, int num_stock, const std::vector<KernelT>& unflipped = {}) {
  auto* typed = static_cast<FunctionT*>(fn);
  std::vector<KernelT> all;
  for (const KernelT* k : typed->kernels()) all.push_back(*k);      // (by value: AddKernel reallocates the function's own vector)
  const int n = static_cast<int>(all.size());
  for (int i = 0; i < std::min(num_stock, n); ++i) {
    KernelT copy = all[i];
    if (copy.exec == nullptr) continue;
    auto data = std::make_shared<GuardData>();
    data->exec = copy.exec;
    data->function = fn->name();
    if (copy.data != nullptr) {
      // a flipped comparison: the kernel it was copied from has the same signature and carries the exec to call
      const bool flipped_copy = static_cast<size_t>(i) < unflipped.size() && unflipped[i].data == nullptr && unflipped[i].exec != nullptr &&
                                unflipped[i].signature->Equals(*copy.signature);
      if (flipped_copy) {
        data->exec = unflipped[i].exec;
        data->flipped = true;
      } else {
        // any other kernel with data of its own: the reference exec runs with a copy of the stock kernel as ctx->kernel()
        data->original = std::make_shared<KernelT>(all[i]);
      }
    }
    copy.exec = GuardedExec;
    if constexpr (std::is_same<KernelT, cp::VectorKernel>::value) {
      if (copy.exec_chunked != nullptr) {
        data->exec_chunked = copy.exec_chunked;
        copy.exec_chunked = GuardedExecChunked;
      }
    }
    copy.data = std::move(data);
    ARROW_RETURN_NOT_OK(typed->AddKernel(std::move(copy)));
  }
  for (int i = num_stock; i < n; ++i) ARROW_RETURN_NOT_OK(typed->AddKernel(all[i]));   // the shim's own kernels: last again
  return Status::OK();
}

// ---- scalar aggregates (round 4): sum / mean / min_max / min / max of the types the shim has no device kernel for
// (strings, decimals, fixed-size binary, half floats, ...).  An aggregate kernel is {init, consume, merge, finalize}
// around a state, and Acero's aggregate nodes build their own KernelContext (no kernel backreference to rely on), so the
// guard lives in the STATE: init (which does receive the kernel, KernelInitArgs::kernel) wraps the reference's state next
// to the reference's vtable; consume refuses a device-resident batch by name and hands host batches on, merge and
// finalize are the reference's.
struct GuardAggData : public cp::KernelState {
  cp::KernelInit init;
  cp::ScalarAggregateConsume consume = nullptr;
  cp::ScalarAggregateMerge merge = nullptr;
  cp::ScalarAggregateFinalize finalize = nullptr;
  std::string function;
};
struct GuardAggState : public cp::KernelState {
  std::unique_ptr<cp::KernelState> stock;
  const GuardAggData* vtable = nullptr;
};

arrow::Result<std::unique_ptr<cp::KernelState>> GuardAggInit(cp::KernelContext* ctx, const cp::KernelInitArgs& args) {
  const auto* data = args.kernel != nullptr ? dynamic_cast<const GuardAggData*>(args.kernel->data.get()) : nullptr;
  if (data == nullptr) return Status::Invalid("arrow_amd: a guarded aggregate kernel was initialised without its kernel");
  auto state = std::make_unique<GuardAggState>();
  state->vtable = data;
  ARROW_ASSIGN_OR_RAISE(state->stock, data->init(ctx, args));
  return state;
}
// `min` / `max` are thin wrappers in the reference: their init dispatches min_max and returns ITS state (MinOrMaxInit,
// aggregate_basic.cc), which is a GuardAggState once min_max is guarded — not something the reference's consume /
// finalize thunks can be handed.  Such an inner state is driven through its own (guarded min_max) vtable, and the
// struct it finalizes to gives up its min or max field the way MinOrMaxFinalize does.
GuardAggState* InnerGuard(GuardAggState* state) { return dynamic_cast<GuardAggState*>(state->stock.get()); }

Status GuardAggConsume(cp::KernelContext* ctx, const cp::ExecSpan& batch) {
  auto* state = static_cast<GuardAggState*>(ctx->state());
  if (GuardAggState* inner = InnerGuard(state)) {
    ctx->SetState(inner);
    const Status st = GuardAggConsume(ctx, batch);
    ctx->SetState(state);
    return st;
  }
  for (const cp::ExecValue& v : batch.values) {
    if (v.is_array() && SpanTouchesRocm(v.array)) {
      return Status::NotImplemented("arrow_amd: ", state->vtable->function, " of ", v.array.type->ToString(), " on device-resident "
                                    "arrays: no device kernel is registered for this type, and the reference's CPU kernel cannot "
                                    "read device memory");
    }
  }
  ctx->SetState(state->stock.get());
  const Status st = state->vtable->consume(ctx, batch);
  ctx->SetState(state);
  return st;
}
Status GuardAggMerge(cp::KernelContext* ctx, cp::KernelState&& src, cp::KernelState* dst) {
  auto& other = static_cast<GuardAggState&>(src);
  auto* mine = static_cast<GuardAggState*>(dst);
  if (GuardAggState* inner = InnerGuard(mine)) {
    GuardAggState* other_inner = InnerGuard(&other);
    if (other_inner == nullptr) return Status::Invalid("arrow_amd: merging a guarded aggregate state with a state of another kind");
    return GuardAggMerge(ctx, std::move(*other_inner), inner);
  }
  cp::KernelState* saved = ctx->state();
  ctx->SetState(mine->stock.get());
  const Status st = mine->vtable->merge(ctx, std::move(*other.stock), mine->stock.get());
  ctx->SetState(saved);
  return st;
}
Status GuardAggFinalize(cp::KernelContext* ctx, arrow::Datum* out) {
  auto* state = static_cast<GuardAggState*>(ctx->state());
  if (GuardAggState* inner = InnerGuard(state)) {
    ctx->SetState(inner);
    const Status st = GuardAggFinalize(ctx, out);
    ctx->SetState(state);
    if (st.ok() && out->is_scalar() && out->scalar()->type->id() == Type::STRUCT) {
      *out = out->scalar_as<arrow::StructScalar>().value[state->vtable->function == "min" ? 0 : 1];
    }
    return st;
  }
  ctx->SetState(state->stock.get());
  const Status st = state->vtable->finalize(ctx, out);
  ctx->SetState(state);
  return st;
}

Status GuardAggregateKernels(cp::Function* fn, int num_stock) {
  auto* typed = static_cast<cp::ScalarAggregateFunction*>(fn);
  std::vector<cp::ScalarAggregateKernel> all;
  for (const cp::ScalarAggregateKernel* k : typed->kernels()) all.push_back(*k);
  const int n = static_cast<int>(all.size());
  for (int i = 0; i < std::min(num_stock, n); ++i) {
    cp::ScalarAggregateKernel copy = all[i];
    if (copy.data != nullptr || copy.consume == nullptr) continue;   // (none of the reference's aggregate kernels carries data)
    auto data = std::make_shared<GuardAggData>();
    data->init = copy.init;
    data->consume = copy.consume;
    data->merge = copy.merge;
    data->finalize = copy.finalize;
    data->function = fn->name();
    copy.init = GuardAggInit;
    copy.consume = GuardAggConsume;
    copy.merge = GuardAggMerge;
    copy.finalize = GuardAggFinalize;
    copy.data = std::move(data);
    ARROW_RETURN_NOT_OK(typed->AddKernel(std::move(copy)));
  }
  for (int i = num_stock; i < n; ++i) ARROW_RETURN_NOT_OK(typed->AddKernel(all[i]));   // the shim's own kernels: last again
  return Status::OK();
}

// the functions whose kernel lists the shim appends to — and the string-search siblings of match_substring, the
// temporal siblings of year .. nanosecond and the nearest string siblings of the lengths, slices and trims (replace_slice,
// reverse, case mapping, padding, swapcase / capitalize / title, replace_substring_regex beside replace_substring,
// binary_join and binary_repeat beside binary_join_element_wise, round_binary beside round, and choose beside case_when), to
// which it adds nothing (every kernel of theirs is the reference's, so every one gets a guard): a device-resident input is
// refused by name instead of being read by a CPU kernel
const char* const kGuardedFunctions[] = {
    "array_filter", "array_take", "array_sort_indices", "equal", "not_equal", "greater", "greater_equal", "less", "less_equal",
    "add", "subtract", "multiply", "divide", "add_checked", "subtract_checked", "multiply_checked", "divide_checked",
    "and_kleene", "or_kleene", "invert", "unique", "value_counts", "dictionary_encode", "indices_nonzero",
    "sum", "mean", "min_max", "min", "max", "coalesce", "is_in", "index_in", "match_substring", "starts_with", "ends_with",
    "match_like", "match_substring_regex", "find_substring", "find_substring_regex", "count_substring",
    "count_substring_regex", "if_else", "year", "quarter", "month", "day", "day_of_week", "day_of_year", "iso_year", "iso_week",
    "hour", "minute", "second", "millisecond", "microsecond", "nanosecond", "is_leap_year", "subsecond", "week", "us_week",
    "us_year", "year_month_day", "iso_calendar", "strftime", "floor_temporal", "ceil_temporal", "round_temporal",
    "binary_length", "utf8_length", "binary_slice", "utf8_slice_codeunits", "binary_replace_slice", "utf8_replace_slice",
    "binary_reverse", "utf8_reverse", "ascii_reverse", "utf8_upper", "utf8_lower", "ascii_upper", "ascii_lower",
    "ascii_trim_whitespace", "ascii_ltrim_whitespace", "ascii_rtrim_whitespace", "utf8_trim_whitespace", "utf8_ltrim_whitespace",
    "utf8_rtrim_whitespace", "ascii_trim", "ascii_ltrim", "ascii_rtrim", "utf8_trim", "utf8_ltrim", "utf8_rtrim",
    "ascii_lpad", "ascii_rpad", "ascii_center", "utf8_lpad", "utf8_rpad", "utf8_center", "ascii_swapcase", "ascii_capitalize",
    "ascii_title", "utf8_swapcase", "utf8_capitalize", "utf8_title", "replace_substring", "replace_substring_regex",
    "binary_join_element_wise", "binary_join", "binary_repeat",
    "negate", "negate_checked", "abs", "abs_checked", "sign", "floor", "ceil", "trunc", "round", "round_to_multiple", "round_binary",
    "case_when", "min_element_wise", "max_element_wise", "choose"};

// before the shim registers anything: how many kernels of each guarded function are the reference's
arrow::Result<std::vector<int>> CountStockKernels(cp::FunctionRegistry* reg) {
  std::vector<int> counts;
  for (const char* name : kGuardedFunctions) {
    ARROW_ASSIGN_OR_RAISE(auto fn, reg->GetFunction(name));
    counts.push_back(fn->num_kernels());
  }
  return counts;
}

// after the shim's registrations
Status InstallDeviceGuards(cp::FunctionRegistry* reg, const std::vector<int>& stock_counts) {
  size_t i = 0;
  for (const char* name : kGuardedFunctions) {
    ARROW_ASSIGN_OR_RAISE(auto fn, reg->GetFunction(name));
    const int num_stock = stock_counts[i++];
    if (fn->kind() == cp::Function::SCALAR) {
      std::vector<cp::ScalarKernel> unflipped;
      const std::string fname = name;
      if (fname == "less" || fname == "less_equal") {
        ARROW_ASSIGN_OR_RAISE(auto source, reg->GetFunction(fname == "less" ? "greater" : "greater_equal"));
        const auto kernels = static_cast<cp::ScalarFunction*>(source.get())->kernels();
        // (that function's stock kernels are still its first num_stock ones: the shim only appends)
        for (int k = 0; k < std::min<int>(num_stock, static_cast<int>(kernels.size())); ++k) unflipped.push_back(*kernels[k]);
      }
      ARROW_RETURN_NOT_OK((GuardKernels<cp::ScalarFunction, cp::ScalarKernel>(fn.get(), num_stock, unflipped)));
    } else if (fn->kind() == cp::Function::VECTOR) {
      ARROW_RETURN_NOT_OK((GuardKernels<cp::VectorFunction, cp::VectorKernel>(fn.get(), num_stock)));
    } else if (fn->kind() == cp::Function::SCALAR_AGGREGATE) {
      ARROW_RETURN_NOT_OK(GuardAggregateKernels(fn.get(), num_stock));
    }
  }
  return Status::OK();
}

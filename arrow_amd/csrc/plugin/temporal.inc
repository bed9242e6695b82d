// year .. iso_week, hour .. nanosecond on device-resident arrays (csrc/temporal.hip).
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).
// ---------------------------------------------------------------- date / time fields
// The reference has one kernel per function and input type (kernels/scalar_temporal_unary.cc: INTERSECTION / PREALLOCATE,
// int64 out; timestamps match by unit whatever their zone).  Every one of them gets a twin: a device-resident array runs
// arx_temporal_component into HBM buffers (the result has no bitmap when the input has none), a host batch the
// reference's exec behind the executor's preallocation contract (RunStockPrepared) — zoned timestamps included, which
// stay the reference's business there; on the device a zone is refused by name (it needs the tz database).
// A reference kernel with an init (day_of_week's DayOfWeekOptions; iso_week keeps week options of its own in a state)
// gets TwinInit (plugin/twin.inc): the reference's state serves host batches, and day_of_week's options are kept for the
// device call; iso_week is called without options and keeps the defaults, which nothing reads.
struct TemporalFunction {
  const char* name;
  int component;   // ARX_TEMPORAL_*
  Fn fn;
};
const TemporalFunction kTemporalFunctions[] = {
    {"year", ARX_TEMPORAL_YEAR, kFnYear}, {"quarter", ARX_TEMPORAL_QUARTER, kFnQuarter}, {"month", ARX_TEMPORAL_MONTH, kFnMonth},
    {"day", ARX_TEMPORAL_DAY, kFnDay}, {"day_of_week", ARX_TEMPORAL_DAY_OF_WEEK, kFnDayOfWeek},
    {"day_of_year", ARX_TEMPORAL_DAY_OF_YEAR, kFnDayOfYear}, {"iso_year", ARX_TEMPORAL_ISO_YEAR, kFnIsoYear},
    {"iso_week", ARX_TEMPORAL_ISO_WEEK, kFnIsoWeek}, {"hour", ARX_TEMPORAL_HOUR, kFnHour}, {"minute", ARX_TEMPORAL_MINUTE, kFnMinute},
    {"second", ARX_TEMPORAL_SECOND, kFnSecond}, {"millisecond", ARX_TEMPORAL_MILLISECOND, kFnMillisecond},
    {"microsecond", ARX_TEMPORAL_MICROSECOND, kFnMicrosecond}, {"nanosecond", ARX_TEMPORAL_NANOSECOND, kFnNanosecond}};

struct TemporalKernelData : public TwinData {
  int component = 0;
};

// ARX_TIME_* of a type of the table, -1 otherwise
int TemporalInputType(const arrow::DataType& t) {
  using arrow::TimeUnit;
  const auto by_unit = [](TimeUnit::type u, int s, int ms, int us, int ns) {
    return u == TimeUnit::SECOND ? s : u == TimeUnit::MILLI ? ms : u == TimeUnit::MICRO ? us : ns;
  };
  switch (t.id()) {
    case Type::DATE32: return ARX_TIME_DATE32;
    case Type::DATE64: return ARX_TIME_DATE64;
    case Type::TIMESTAMP:
      return by_unit(static_cast<const arrow::TimestampType&>(t).unit(), ARX_TIME_TIMESTAMP_S, ARX_TIME_TIMESTAMP_MS, ARX_TIME_TIMESTAMP_US,
                     ARX_TIME_TIMESTAMP_NS);
    case Type::TIME32: return by_unit(static_cast<const arrow::Time32Type&>(t).unit(), ARX_TIME_TIME32_S, ARX_TIME_TIME32_MS, -1, -1);
    case Type::TIME64: return by_unit(static_cast<const arrow::Time64Type&>(t).unit(), -1, -1, ARX_TIME_TIME64_US, ARX_TIME_TIME64_NS);
    default: return -1;
  }
}

Status TemporalExecNP(cp::KernelContext* ctx, const cp::ExecSpan& batch, cp::ExecResult* out) {
  const auto* kd = TwinDataOf<TemporalKernelData>(ctx->kernel());
  if (kd == nullptr) return TwinWithoutData();
  auto* state = kd->stock_init ? static_cast<ShimState<cp::DayOfWeekOptions>*>(ctx->state()) : nullptr;
  if (kd->stock_init && state == nullptr) return Status::Invalid("arrow_amd: ", kFnNames[kd->fn], " ran without its state");
  const ShimState<cp::DayOfWeekOptions>* dow = kd->component == ARX_TEMPORAL_DAY_OF_WEEK ? state : nullptr;
  if (!batch[0].is_array() || !SpanTouchesRocm(batch[0].array)) {
    // ---- a host batch (or a scalar): the executor's preallocation, then the reference's exec
    return RunStockPrepared(kd->fn, kd->stock_exec, state != nullptr ? std::optional<cp::KernelState*>(state->stock.get()) : std::nullopt,
                            8, TwinValidity::kIntersection, ctx, batch, out);
  }
  const ArraySpan& rows = batch[0].array;
  const arrow::DataType& type = *rows.type;
  if (type.id() == Type::TIMESTAMP && !static_cast<const arrow::TimestampType&>(type).timezone().empty()) {
    return Status::NotImplemented("arrow_amd: ", kFnNames[kd->fn], " of ", type.ToString(), " on device-resident arrays: time zones "
                                  "need the tz database, which has no device kernel");
  }
  const int in_type = TemporalInputType(type);
  if (in_type < 0) return Status::Invalid("arrow_amd: ", kFnNames[kd->fn], " twin matched ", type.ToString());
  const int64_t n = rows.length;
  hipStream_t st;
  ARROW_RETURN_NOT_OK(t_scratch.Stream(&st));
  ArxSpan vs{};
  ARROW_RETURN_NOT_OK(DeviceSpan(rows, &vs));
  if (vs.null_count == 0) vs.validity = nullptr;
  ArrayData* out_arr = out->array_data().get();
  out_arr->buffers.assign(2, nullptr);
  ARROW_ASSIGN_OR_RAISE(out_arr->buffers[1], AllocDevice(std::max<int64_t>(n * 8, 8)));
  std::shared_ptr<Buffer> valid;
  if (vs.validity != nullptr) {
    ARROW_ASSIGN_OR_RAISE(valid, AllocDevice(BitmapBytes(n)));
  }
  ARROW_RETURN_NOT_OK(FromArx(arx_temporal_component(kd->component, in_type, &vs, n, dow != nullptr ? dow->options.week_start : 1,
                                                     dow != nullptr ? (dow->options.count_from_zero ? 1 : 0) : 1,
                                                     reinterpret_cast<void*>(out_arr->buffers[1]->mutable_address()),
                                                     valid != nullptr ? reinterpret_cast<void*>(valid->mutable_address()) : nullptr, st)));
  out_arr->null_count = 0;
  if (valid != nullptr) {
    if (vs.null_count > 0) {
      out_arr->null_count = vs.null_count;
      HIP_RETURN_NOT_OK(hipStreamSynchronize(st));
    } else {
      ARROW_ASSIGN_OR_RAISE(out_arr->null_count, DeviceNullCount(*valid, n, st));   // (synchronizes)
    }
    if (out_arr->null_count != 0) out_arr->buffers[0] = valid;
  } else {
    HIP_RETURN_NOT_OK(hipStreamSynchronize(st));   // (this thread's scratch may be released after return)
  }
  CountGpu(kd->fn);
  return Status::OK();
}

// one twin per function and input type of the reference's lists, appended after the reference's kernels (dispatch takes
// the last match); the reference's own kernels stay behind the device guard (plugin/device_guard.inc)
Status RegisterTemporal(cp::FunctionRegistry* reg) {
  using arrow::TimeUnit;
  const std::vector<ValueType> calendar = {
      ValueType(arrow::date32()), ValueType(arrow::date64()),
      ValueType(arrow::timestamp(TimeUnit::SECOND), cp::InputType(cp::match::TimestampTypeUnit(TimeUnit::SECOND))),
      ValueType(arrow::timestamp(TimeUnit::MILLI), cp::InputType(cp::match::TimestampTypeUnit(TimeUnit::MILLI))),
      ValueType(arrow::timestamp(TimeUnit::MICRO), cp::InputType(cp::match::TimestampTypeUnit(TimeUnit::MICRO))),
      ValueType(arrow::timestamp(TimeUnit::NANO), cp::InputType(cp::match::TimestampTypeUnit(TimeUnit::NANO)))};
  std::vector<ValueType> time_of_day(calendar.begin() + 2, calendar.end());
  time_of_day.emplace_back(arrow::time32(TimeUnit::SECOND), cp::InputType(cp::match::Time32TypeUnit(TimeUnit::SECOND)));
  time_of_day.emplace_back(arrow::time32(TimeUnit::MILLI), cp::InputType(cp::match::Time32TypeUnit(TimeUnit::MILLI)));
  time_of_day.emplace_back(arrow::time64(TimeUnit::MICRO), cp::InputType(cp::match::Time64TypeUnit(TimeUnit::MICRO)));
  time_of_day.emplace_back(arrow::time64(TimeUnit::NANO), cp::InputType(cp::match::Time64TypeUnit(TimeUnit::NANO)));
  for (const TemporalFunction& f : kTemporalFunctions) {
    ARROW_RETURN_NOT_OK(AppendTwins(
        reg, f.name, f.component <= ARX_TEMPORAL_ISO_WEEK ? calendar : time_of_day,
        [](const auto& t) { return std::vector<arrow::TypeHolder>{t}; },
        [=](const ValueType& vt, cp::ScalarKernel* twin) -> arrow::Result<bool> {
          auto data = std::make_shared<TemporalKernelData>();
          data->component = f.component;
          ARROW_RETURN_NOT_OK(InstallTwin(f.name, vt, twin, f.component != ARX_TEMPORAL_DAY_OF_WEEK || twin->init, std::move(data), f.fn,
                                          TwinInit<cp::DayOfWeekOptions>, TemporalExecNP,
                                          cp::KernelSignature::Make({vt.match}, cp::OutputType(arrow::int64()))));
          return true;
        }));
  }
  return Status::OK();
}

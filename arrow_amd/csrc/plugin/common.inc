// Counters, status mapping, per-thread device scratch, host staging, kernel state shared by the shims.
// Part of the Arrow registration shim: included by ../arrow_plugin.cc inside its anonymous
// namespace (one translation unit; the split is for reading, not for linkage).

std::atomic<int64_t> g_gpu_calls{0};
std::atomic<int64_t> g_stock_calls{0};
std::atomic<int64_t> g_min_rows{1 << 16};
// Element-wise kernels (greater, cast) on HOST arrays move more bytes over PCIe than the CPU needs
// time to compute them (100M rows, one MI355X box: greater 38 ms staged vs 24 ms stock; cast 27 vs
// 33 ms; filter 17 vs 116 ms; sort 46 ms vs 14.8 s — scripts/exp_plugin_host_staging.py), so by
// default they stay on Arrow's stock kernels; device-resident arrays always run on the GPU.
std::atomic<int64_t> g_min_rows_streaming{INT64_MAX};
// Device-resident filters of at most this many rows take the single-synchronisation path (worst-case output
// allocation, count -> compact back to back, one read-back instead of three round trips).  On by default for
// morsel-sized inputs (<= 1M rows) since the round-2 A/B on an MI355X (profiles/r02_a_acero_morsel_ab.txt: the 4M-row
// Acero plan 33.2 -> 32.9 ms single-threaded, 15.6 -> 14.7 ms threaded, never slower); larger arrays keep the exact-size
// allocation.  arrow_amd_plugin_set_filter_morsel_rows() / ARROW_AMD_FILTER_MORSEL_ROWS change it (0 = off).
std::atomic<int64_t> g_filter_morsel_rows{[] {
  const char* env = std::getenv("ARROW_AMD_FILTER_MORSEL_ROWS");
  return env != nullptr ? static_cast<int64_t>(std::strtoll(env, nullptr, 10)) : int64_t(1) << 20;
}()};

// Parquet: Snappy chunks of fixed-width columns are read raw and their PLAIN value pages decompressed on the device
// (ARROW_AMD_PARQUET_DEVICE_SNAPPY=0 / arrow_amd_plugin_set_parquet_device_snappy(0): the reference's PageReader
// decompresses every page on the host, as before)
std::atomic<bool> g_parquet_pinned_staging{true};
std::atomic<bool> g_parquet_device_levels{true};   // V2 chunks: definition levels' run headers walked on the device
std::atomic<int> g_parquet_read_threads{4};       // threads that share the read of one large column chunk
std::atomic<int64_t> g_parquet_read_part_bytes{int64_t(1) << 23};   // ... at least this many bytes each
std::atomic<bool> g_parquet_device_snappy{[] {
  const char* env = std::getenv("ARROW_AMD_PARQUET_DEVICE_SNAPPY");
  return env == nullptr || std::strtoll(env, nullptr, 10) != 0;
}()};
std::atomic<int64_t> g_parquet_device_snappy_pages{0};
// GZIP chunks take the same raw route (arx_gzip_decompress_pages); arrow_amd_plugin_set_parquet_device_gzip(0) turns it off
std::atomic<bool> g_parquet_device_gzip{true};
std::atomic<int64_t> g_parquet_device_gzip_pages{0};
std::atomic<int64_t> g_parquet_copied_pages{0};   // device-route pages whose body was NOT a slice of the chunk read

// aggregate_rocm: device-resident batches without nulls are only remembered when they arrive and copied into the
// node's staging columns this many rows at a time, by one launch (arx_copy_segments)
std::atomic<int64_t> g_aggregate_flush_rows{[] {
  const char* env = std::getenv("ARROW_AMD_AGGREGATE_FLUSH_ROWS");
  return env != nullptr ? std::max<int64_t>(1, std::strtoll(env, nullptr, 10)) : int64_t(1) << 21;
}()};
// aggregate_rocm: a device-resident batch of at least this many rows is consumed where it lies (no copy into the staging
// columns); table_source_rocm delivers such batches
std::atomic<int64_t> g_aggregate_direct_rows{int64_t(1) << 22};
std::atomic<int64_t> g_aggregate_direct_batches{0};
// aggregate_rocm: a plan whose whole input is one run of device slices (>= range_min_rows rows, no nulls, sums / counts
// only) goes through the range-partitioned state (arx_groupby_range_*) when the sampled key range suits it
std::atomic<bool> g_aggregate_range_state{true};
std::atomic<int64_t> g_aggregate_range_min_rows{int64_t(1) << 22};
std::atomic<int64_t> g_aggregate_range_sample_rows{int64_t(1) << 20};
std::atomic<int64_t> g_aggregate_range_plans{0};
std::atomic<int64_t> g_aggregate_range_declined{0};
// select_k_unstable of a device array by a threshold instead of a sort (plugin/rank.inc): the column's row floor, how often it ran
std::atomic<int64_t> g_select_k_min_rows{int64_t(1) << 22};
std::atomic<int64_t> g_select_k_threshold_runs{0};
// the C++ sharded group-by (plugin/sharded.inc) on the range-partitioned state: on / off, one rank's row floor, runs / declines
std::atomic<bool> g_sharded_range_state{true};
std::atomic<int64_t> g_sharded_range_min_rows{int64_t(1) << 22};
std::atomic<int64_t> g_sharded_range_runs{0};
std::atomic<int64_t> g_sharded_range_declined{0};
// the C++ sharded sort (plugin/sharded_sort.inc): the records form for null-free shards (default on), its sampled key window /
// splitter histogram (one tile of 8192 rows in 2^shift when the longest shard has min_rows rows; shift 0: never), how often
// the records form ran
std::atomic<bool> g_sharded_sort_records{true};
std::atomic<int> g_sharded_sort_sample_shift{4};
std::atomic<int64_t> g_sharded_sort_sample_min_rows{int64_t(1) << 20};
std::atomic<int64_t> g_sharded_sort_records_runs{0};
// coalesce_rocm: device batches are joined until they hold this many rows
std::atomic<int64_t> g_coalesce_rows{int64_t(1) << 26};
std::atomic<int64_t> g_coalesced_batches{0};
// table_source_rocm: rows per batch when the caller left TableSourceNodeOptions::max_batch_size at its default
std::atomic<int64_t> g_table_source_rows{int64_t(1) << 27};
// result columns of a megabyte or more leave the device into pooled page-locked host buffers (0: the query's memory pool)
std::atomic<bool> g_pinned_results{[] {
  const char* env = std::getenv("ARROW_AMD_PINNED_RESULTS");
  return env == nullptr || std::strtoll(env, nullptr, 10) != 0;
}()};
std::atomic<bool> g_results_kernel_copy{true};   // column-sized result copies by arx_buffer_copy instead of hipMemcpyAsync (A/B)
std::atomic<bool> g_aggregate_device_output{false};   // aggregate_rocm: device-resident input -> device-resident result columns
std::atomic<bool> g_aggregate_stage_nulls{true};   // aggregate_rocm: device batches WITH nulls are staged like the others (0: consumed one by one)
std::atomic<int64_t> g_aggregate_flushes{0};
std::atomic<int64_t> g_string_key_hash_bits{64};        // aggregate_rocm: bits of the var-width keys' hash (0: the exact chunk columns only; < 64 forces collisions in tests)
std::atomic<int64_t> g_string_key_hash_collisions{0};   // batches regrouped by the exact chunk columns after a verified collision

// per-function call counters: which exec actually ran (the GPU tests assert on these so that a
// silent route through the stock CPU kernel is a test failure, not a pass)
enum Fn { kFnFilter = 0, kFnTake, kFnGreater, kFnSort, kFnCast, kFnHashSum, kFnAdd, kFnBoolean, kFnCompare, kFnParquet,
          kFnReduce, kFnOrderBy, kFnTakeColumns, kFnUnique, kFnCoalesce, kFnIsIn, kFnIndexIn, kFnHashJoin,
          kFnMatchSubstring, kFnStartsWith, kFnEndsWith, kFnIfElse, kFnYear, kFnQuarter, kFnMonth, kFnDay, kFnDayOfWeek,
          kFnDayOfYear, kFnIsoYear, kFnIsoWeek, kFnHour, kFnMinute, kFnSecond, kFnMillisecond, kFnMicrosecond, kFnNanosecond,
          kFnBinaryLength, kFnUtf8Length, kFnBinarySlice, kFnUtf8SliceCodeunits, kFnAsciiTrimWhitespace, kFnAsciiLtrimWhitespace,
          kFnAsciiRtrimWhitespace, kFnUtf8TrimWhitespace, kFnUtf8LtrimWhitespace, kFnUtf8RtrimWhitespace, kFnAsciiTrim, kFnAsciiLtrim,
          kFnAsciiRtrim, kFnUtf8Trim, kFnUtf8Ltrim, kFnUtf8Rtrim, kFnCompareString, kFnReplaceSubstring, kFnUnaryArith, kFnRound,
          kFnBinaryJoinElementWise, kFnCaseWhen, kFnMinElementWise, kFnMaxElementWise,
          kNumFn };
const char* const kFnNames[kNumFn] = {"array_filter", "array_take", "greater", "array_sort_indices",
                                      "cast", "hash_sum", "add", "boolean", "compare", "parquet", "reduce", "order_by",
                                      "take_columns", "unique", "coalesce", "is_in", "index_in", "hashjoin",
                                      "match_substring", "starts_with", "ends_with", "if_else", "year", "quarter", "month", "day",
                                      "day_of_week", "day_of_year", "iso_year", "iso_week", "hour", "minute", "second",
                                      "millisecond", "microsecond", "nanosecond", "binary_length", "utf8_length", "binary_slice",
                                      "utf8_slice_codeunits", "ascii_trim_whitespace", "ascii_ltrim_whitespace",
                                      "ascii_rtrim_whitespace", "utf8_trim_whitespace", "utf8_ltrim_whitespace",
                                      "utf8_rtrim_whitespace", "ascii_trim", "ascii_ltrim", "ascii_rtrim", "utf8_trim", "utf8_ltrim",
                                      "utf8_rtrim", "compare_string", "replace_substring", "unary_arith", "round",
                                      "binary_join_element_wise", "case_when", "min_element_wise", "max_element_wise"};
std::atomic<int64_t> g_fn_gpu[kNumFn];
std::atomic<int64_t> g_fn_stock[kNumFn];
void CountGpu(Fn f) {
  g_gpu_calls.fetch_add(1, std::memory_order_relaxed);
  g_fn_gpu[f].fetch_add(1, std::memory_order_relaxed);
}
void CountStock(Fn f) {
  g_stock_calls.fetch_add(1, std::memory_order_relaxed);
  g_fn_stock[f].fetch_add(1, std::memory_order_relaxed);
}
thread_local std::string t_error;

Status FromArx(int rc) {
  if (rc == ARX_OK) return Status::OK();
  const std::string msg = arx_last_error();
  switch (rc) {
    case ARX_INVALID: return Status::Invalid(msg);
    case ARX_CAPACITY_ERROR: return Status::CapacityError(msg);
    case ARX_INDEX_ERROR: return Status::IndexError(msg);
    case ARX_NOT_IMPLEMENTED: return Status::NotImplemented(msg);
    case ARX_OUT_OF_MEMORY: return Status::OutOfMemory(msg);
    default: return Status::UnknownError(msg);
  }
}

#define HIP_RETURN_NOT_OK(call)                                                        \
  do {                                                                                 \
    hipError_t e__ = (call);                                                           \
    if (e__ != hipSuccess)                                                             \
      return Status::IOError("HIP: ", hipGetErrorString(e__), " in " #call);           \
  } while (0)

// ---------------------------------------------------------------- per-thread device scratch
// Kernel::exec may be called concurrently from Acero's thread pool with the same const Kernel*
// (SURVEY.md 8b): every host thread owns a stream and a handful of growable HBM staging slots.
// This thread's stream in a TRIVIALLY DESTRUCTIBLE thread_local: ~RocmBuffer reads it, and buffers outlive threads (a last
// reference dropped during thread exit or interpreter teardown must not touch a destroyed DeviceScratch — ADVICE r3).
thread_local hipStream_t t_stream = nullptr;

class DeviceScratch {
 public:
  ~DeviceScratch() {
    for (auto& s : slots_) {
      if (s.ptr) (void)hipFree(s.ptr);
    }
    // the stream is deliberately NOT destroyed: RocmBuffers remember the stream of the thread that allocated them
    // (they wait for it before their block is reused) and may outlive this thread
  }
  hipStream_t PeekStream() const { return stream_; }
  Status Stream(hipStream_t* out) {
    if (!stream_) {
      HIP_RETURN_NOT_OK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
      t_stream = stream_;
    }
    *out = stream_;
    return Status::OK();
  }
  Status Get(int slot, size_t bytes, void** out) {
    if (slots_.size() <= static_cast<size_t>(slot)) slots_.resize(slot + 1);
    Slot& s = slots_[slot];
    bytes = (bytes + 255) & ~size_t(255);
    if (s.size < bytes) {
      if (s.ptr) HIP_RETURN_NOT_OK(hipFree(s.ptr));
      s.ptr = nullptr;
      s.size = 0;
      const size_t want = std::max<size_t>(bytes + bytes / 4, 1 << 20);
      HIP_RETURN_NOT_OK(hipMalloc(&s.ptr, want));
      s.size = want;
    }
    *out = s.ptr;
    return Status::OK();
  }

 private:
  struct Slot { void* ptr = nullptr; size_t size = 0; };
  std::vector<Slot> slots_;
  hipStream_t stream_ = nullptr;
};
thread_local DeviceScratch t_scratch;

// Page-locked host staging, one growable block per host thread, kept from call to call: bytes the device reads once
// (a Parquet column chunk) land here and cross PCIe in ONE copy that the DMA engines read directly.  Keeping the block
// matters more than its being page-locked: a fresh buffer pays a page fault per 4 KB the first time it is written.
// The caller must have waited for the copy that reads the block before the next Reserve of the same thread.
class PinnedStaging {
 public:
  ~PinnedStaging() {
    if (ptr_) (void)hipHostFree(ptr_);
  }
  Status Reserve(size_t bytes, uint8_t** out) {
    if (size_ < bytes) {
      if (ptr_) HIP_RETURN_NOT_OK(hipHostFree(ptr_));
      ptr_ = nullptr;
      size_ = 0;
      const size_t want = std::max<size_t>(bytes + bytes / 4, size_t(1) << 20);
      HIP_RETURN_NOT_OK(hipHostMalloc(&ptr_, want, hipHostMallocDefault));
      size_ = want;
    }
    *out = static_cast<uint8_t*>(ptr_);
    return Status::OK();
  }
  // give back a block that one unusually large chunk made huge (called with no copy in flight)
  void Trim(size_t keep_at_most) {
    if (size_ > keep_at_most && ptr_ != nullptr) {
      (void)hipHostFree(ptr_);
      ptr_ = nullptr;
      size_ = 0;
    }
  }

 private:
  void* ptr_ = nullptr;
  size_t size_ = 0;
};
thread_local PinnedStaging t_pinned;

enum Slot { kValues = 0, kValidity, kArg2, kArg2Validity, kOutData, kOutValidity, kWs, kCounter, kBinWs, kFlag };

// Upload the logical range of a fixed-width (or boolean) ArraySpan.  The device copy keeps the
// sub-byte part of the offset (offset % 8) so that one logical offset addresses both buffers.
Status Upload(const ArraySpan& a, int byte_width_or_0_for_bool, int data_slot, int validity_slot,
              hipStream_t st, ArxSpan* out) {
  const int64_t o8 = a.offset % 8;
  const int64_t first = a.offset - o8;
  out->offset = o8;
  out->length = a.length;
  out->null_count = a.null_count;
  out->validity = nullptr;
  out->data = nullptr;
  const int64_t span_elems = o8 + a.length;
  if (a.buffers[1].data != nullptr && a.length > 0) {
    const uint8_t* src;
    size_t bytes;
    if (byte_width_or_0_for_bool == 0) {
      src = a.buffers[1].data + first / 8;
      bytes = static_cast<size_t>(arrow::bit_util::BytesForBits(span_elems));
    } else {
      src = a.buffers[1].data + first * byte_width_or_0_for_bool;
      bytes = static_cast<size_t>(span_elems) * byte_width_or_0_for_bool;
    }
    void* d = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(data_slot, bytes + 16, &d));
    HIP_RETURN_NOT_OK(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, st));
    out->data = d;
  }
  if (a.buffers[0].data != nullptr && a.null_count != 0 && a.length > 0) {
    const size_t bytes = static_cast<size_t>(arrow::bit_util::BytesForBits(span_elems));
    void* d = nullptr;
    ARROW_RETURN_NOT_OK(t_scratch.Get(validity_slot, bytes + 16, &d));
    HIP_RETURN_NOT_OK(hipMemcpyAsync(d, a.buffers[0].data + first / 8, bytes, hipMemcpyHostToDevice, st));
    out->validity = d;
  } else if (a.null_count != 0 && a.buffers[0].data == nullptr) {
    out->null_count = 0;  // no bitmap: all valid
  }
  return Status::OK();
}

bool IsHost(const ArraySpan& a) {
  for (int i = 0; i < 2; ++i) {
    if (a.buffers[i].owner != nullptr && *a.buffers[i].owner != nullptr &&
        !(*a.buffers[i].owner)->is_cpu()) {
      return false;
    }
  }
  return true;
}

int FixedByteWidth(const arrow::DataType& t) {
  switch (t.id()) {
    case Type::INT8: case Type::UINT8: return 1;
    case Type::INT16: case Type::UINT16: case Type::HALF_FLOAT: return 2;
    case Type::INT32: case Type::UINT32: case Type::FLOAT: case Type::DATE32: case Type::TIME32:
    case Type::INTERVAL_MONTHS: case Type::DECIMAL32: return 4;
    case Type::INT64: case Type::UINT64: case Type::DOUBLE: case Type::DATE64: case Type::TIME64:
    case Type::TIMESTAMP: case Type::DURATION: case Type::INTERVAL_DAY_TIME: case Type::DECIMAL64: return 8;
    case Type::DECIMAL128: case Type::INTERVAL_MONTH_DAY_NANO: return 16;
    case Type::DECIMAL256: return 32;
    case Type::FIXED_SIZE_BINARY: {
      const int w = static_cast<const arrow::FixedSizeBinaryType&>(t).byte_width();
      return (w == 1 || w == 2 || w == 4 || w == 8 || w == 16 || w == 32) ? w : 0;  // other widths: stock kernel
    }
    default: return 0;
  }
}

// bytes per offset of a binary / utf8 type: 8 for the large forms, 4 otherwise
int BinaryOffsetWidth(Type::type id) { return (id == Type::LARGE_STRING || id == Type::LARGE_BINARY) ? 8 : 4; }

// ---------------------------------------------------------------- state = stock state + options
template <typename Options>
struct ShimState : public cp::KernelState {
  std::unique_ptr<cp::KernelState> stock;
  Options options;
};

struct StockKernel {
  cp::KernelInit init;
  cp::ArrayKernelExec exec = nullptr;
  cp::VectorKernel::ChunkedExec exec_chunked = nullptr;
};

// count and run a stock exec (an ArrayKernelExec or a ChunkedExec); a stock state, when given, is installed around the
// call and ours restored whatever the call returns
template <class Exec, class Batch, class Out>
Status RunStock(Fn fn, Exec exec, std::optional<cp::KernelState*> stock_state, cp::KernelContext* ctx, const Batch& batch,
                Out* out) {
  CountStock(fn);
  if (!stock_state.has_value()) return exec(ctx, batch, out);
  cp::KernelState* mine = ctx->state();
  ctx->SetState(*stock_state);
  Status st = exec(ctx, batch, out);
  ctx->SetState(mine);
  return st;
}
Status RunStock(Fn fn, const StockKernel& k, cp::KernelState* stock_state, cp::KernelContext* ctx,
                const cp::ExecSpan& batch, cp::ExecResult* out) {
  return RunStock(fn, k.exec, std::optional<cp::KernelState*>(stock_state), ctx, batch, out);
}

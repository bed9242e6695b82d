// Lengths and slices of utf8 / binary columns and their large forms: binary_length, utf8_length, binary_slice and
// utf8_slice_codeunits with step 1 (compute/kernels/scalar_string_ascii.cc / scalar_string_utf8.cc).  The first scalar
// kernels here whose result is a variable-length column; the take of binary.hip is the model: lengths -> scan ->
// offsets -> copy, with the scan and the copy kernel of binary.hip itself (binary_scan_copy.h).
//
// Units.  ARX_STRING_UNIT_BYTES counts and slices bytes: offset arithmetic, no data byte is read before the copy.
// ARX_STRING_UNIT_CODEPOINTS counts and slices codepoints.  A codepoint starts at every byte that is not 0b10xxxxxx (a
// LEAD below), whether or not the row is valid UTF-8, and positions are defined so that they never leave the row:
//   codepoint k >= 0        begins at the (k + 1)-th lead of the row, or at the row's end if it has fewer;
//   k >= 1 from the end     begins at the k-th lead counted backwards, or at the row's start if it has fewer.
// A slice [start, stop) resolves each bound by its sign (stop = INT64_MAX: the row's end), then begin = min(begin, end).
// A non-negative bound walks from the row's front and a negative one from its back, so neither needs the row's count and
// slice(0, 2) of a long row reads its first granule only.  Valid UTF-8 gives Python's s[start:stop].
//
// Granule rule (as match_substring.hip): a load touches only an aligned 16-byte granule that holds at least one byte of
// the row.  The leads of a granule are bit 7 of the bytes of two 64-bit masks; counting is a popcount, the k-th lead a
// few clears of the lowest bit.
//
// Two forms of the codepoint walk.
//   rows  : one lane per row.  Short rows: a lane reads one or two granules.
//   waves : one wave per row; the lanes take 64 consecutive granules (1 KiB) a step, an inclusive scan of their counts
//           and one ballot find the lane and the byte of the k-th lead.  Long or skewed rows: a lane of the rows form
//           would walk its row alone while 63 idle.  A wave takes 64 consecutive rows one after the other and lane i
//           keeps row i's result, so results are stored coalesced and a sum gets one atomic per 64 rows in both forms.
// Auto takes the waves form from a mean row size (data_bytes_hint / length) of kWavesPathMeanRow bytes on (string_rows.h).
//
// Slicing is two calls, since the output size depends on the data: arx_string_slice_offsets writes every row's source
// begin into the workspace and its length into out_offsets, adds the lengths of every kBinRows rows into the
// workspace's sums (one atomic a wave), scans (bin_scan_lengths) and returns the total; arx_string_slice_data copies
// (bin_copy_rows).  The output never exceeds the input, so int32 offsets cannot overflow.
#include "string_rows.h"

namespace arx {

namespace {

constexpr int64_t kNoStop = INT64_MAX;
constexpr int kLengthMaxBlocks = 1 << 20;   // workgroups of a binary_length launch (a workgroup strides over what is left)

std::atomic<int64_t> g_slice_row_launches{0}, g_slice_wave_launches{0};

// bit 7 of byte j of lo / hi set: byte j / 8 + j of the granule belongs to the row and is a lead
struct Leads {
  uint64_t lo, hi;
};
__device__ __forceinline__ int lead_count(Leads l) { return __popcll(l.lo) + __popcll(l.hi); }

// the leads of the aligned granule at address g among the row's bytes [s, e) (addresses); g + 16 > s and g < e
__device__ __forceinline__ Leads granule_leads(uint64_t g, uint64_t s, uint64_t e) {
  const uint4 q = *reinterpret_cast<const uint4*>(g);
  const uint64_t lo = q.x | (static_cast<uint64_t>(q.y) << 32), hi = q.z | (static_cast<uint64_t>(q.w) << 32);
  Leads l;
  // a continuation byte has bit 7 set and bit 6 clear
  l.lo = ~(lo & ~(lo << 1)) & kBit7;
  l.hi = ~(hi & ~(hi << 1)) & kBit7;
  if (g < s || g + 16 > e) {
    const int64_t from = g < s ? static_cast<int64_t>(s - g) : 0, to = g + 16 > e ? static_cast<int64_t>(e - g) : 16;
    l.lo &= byte_range_bit7(from, to);
    l.hi &= byte_range_bit7(from - 8, to - 8);
  }
  return l;
}

// the byte (0 .. 15) of the k-th lead of the granule counted from its first byte, 1 <= k <= lead_count(l)
__device__ __forceinline__ int kth_lead(Leads l, int k) {
  const int in_lo = __popcll(l.lo);
  uint64_t w = l.lo;
  int base = 0;
  if (k > in_lo) {
    w = l.hi;
    k -= in_lo;
    base = 8;
  }
  for (; k > 1; --k) w &= w - 1;
  return base + ((__ffsll(static_cast<unsigned long long>(w)) - 1) >> 3);
}

// ---------------------------------------------------------------- one lane per row
// the address of the (k + 1)-th lead of [s, e), or e
__device__ __forceinline__ uint64_t lane_forward(uint64_t s, uint64_t e, uint64_t k) {
  if (k >= e - s) return e;               // (a row has at most as many leads as bytes)
  int64_t need = static_cast<int64_t>(k) + 1;
  for (uint64_t g = s & ~uint64_t(15); g < e; g += 16) {
    const Leads l = granule_leads(g, s, e);
    const int c = lead_count(l);
    if (c >= need) return g + kth_lead(l, static_cast<int>(need));
    need -= c;
  }
  return e;
}

// the address of the k-th lead of [s, e) counted backwards (k >= 1), or s
__device__ __forceinline__ uint64_t lane_backward(uint64_t s, uint64_t e, uint64_t k) {
  if (s == e || k > e - s) return s;
  int64_t need = static_cast<int64_t>(k);
  const uint64_t g_first = s & ~uint64_t(15);
  for (uint64_t g = (e - 1) & ~uint64_t(15);; g -= 16) {
    const Leads l = granule_leads(g, s, e);
    const int c = lead_count(l);
    if (c >= need) return g + kth_lead(l, c - static_cast<int>(need) + 1);
    need -= c;
    if (g == g_first) break;
  }
  return s;
}

__device__ __forceinline__ int64_t lane_count(uint64_t s, uint64_t e) {
  int64_t c = 0;
  for (uint64_t g = s & ~uint64_t(15); g < e; g += 16) c += lead_count(granule_leads(g, s, e));
  return c;
}

// ---------------------------------------------------------------- one wave per row (s, e, k wave-uniform)
__device__ __forceinline__ uint64_t wave_forward(uint64_t s, uint64_t e, uint64_t k) {
  if (k >= e - s) return e;
  const int lane = lane_id();
  int64_t need = static_cast<int64_t>(k) + 1;
  for (uint64_t base = s & ~uint64_t(15); base < e; base += 16 * kWave) {
    const uint64_t g = base + 16 * static_cast<uint64_t>(lane);
    Leads l{0, 0};
    if (g < e) l = granule_leads(g, s, e);
    const uint32_t c = static_cast<uint32_t>(lead_count(l));
    const uint32_t incl = wave_inclusive_scan_u32(c);
    const int64_t total = __shfl(incl, 63, 64);
    if (total >= need) {
      const int src = __ffsll(static_cast<unsigned long long>(__ballot(static_cast<int64_t>(incl) >= need))) - 1;
      uint64_t pos = 0;
      if (lane == src) pos = g + kth_lead(l, static_cast<int>(need - (incl - c)));
      return shfl_u64(pos, src);
    }
    need -= total;
  }
  return e;
}

__device__ __forceinline__ uint64_t wave_backward(uint64_t s, uint64_t e, uint64_t k) {
  if (s == e || k > e - s) return s;
  const int lane = lane_id();
  int64_t need = static_cast<int64_t>(k);
  const uint64_t g_first = s & ~uint64_t(15);
  // lane 0 takes the row's last granule, lane 1 the one before: lane order is the order of the walk
  for (uint64_t top = (e - 1) & ~uint64_t(15);; top -= 16 * kWave) {
    const uint64_t back = 16 * static_cast<uint64_t>(lane);
    const bool active = top - g_first >= back;
    const uint64_t g = top - back;
    Leads l{0, 0};
    if (active) l = granule_leads(g, s, e);
    const uint32_t c = static_cast<uint32_t>(lead_count(l));
    const uint32_t incl = wave_inclusive_scan_u32(c);
    const int64_t total = __shfl(incl, 63, 64);
    if (total >= need) {
      const int src = __ffsll(static_cast<unsigned long long>(__ballot(static_cast<int64_t>(incl) >= need))) - 1;
      uint64_t pos = 0;
      if (lane == src) pos = g + kth_lead(l, static_cast<int>(c - (need - (incl - c)) + 1));
      return shfl_u64(pos, src);
    }
    need -= total;
    if (top - g_first < 16 * kWave) break;
  }
  return s;
}

__device__ __forceinline__ int64_t wave_count(uint64_t s, uint64_t e) {
  uint64_t c = 0;
  for (uint64_t g = (s & ~uint64_t(15)) + 16 * static_cast<uint64_t>(lane_id()); g < e; g += 16 * kWave) {
    c += static_cast<uint64_t>(lead_count(granule_leads(g, s, e)));
  }
  return static_cast<int64_t>(wave_reduce_sum_u64(c));
}

// ---------------------------------------------------------------- bounds -> [begin, end) of a row
struct Range {
  int64_t begin, end;   // indices into the data buffer
};

// bytes: Python's slice of a row of `len` bytes
__device__ __forceinline__ int64_t byte_bound(int64_t x, int64_t len) {
  return x >= 0 ? (x < len ? x : len) : (len + x > 0 ? len + x : 0);
}
__device__ __forceinline__ Range byte_range(int64_t s_off, int64_t e_off, int64_t start, int64_t stop) {
  const int64_t len = e_off - s_off;
  Range r;
  r.end = s_off + (stop == kNoStop ? len : byte_bound(stop, len));
  r.begin = s_off + byte_bound(start, len);
  if (r.begin > r.end) r.begin = r.end;
  return r;
}

// codepoints: WAVE = the row is the wave's (all lanes call), else the lane's
template <bool WAVE>
__device__ __forceinline__ uint64_t codepoint_bound(uint64_t s, uint64_t e, int64_t x) {
  if (x >= 0) return WAVE ? wave_forward(s, e, static_cast<uint64_t>(x)) : lane_forward(s, e, static_cast<uint64_t>(x));
  const uint64_t k = uint64_t(0) - static_cast<uint64_t>(x);
  return WAVE ? wave_backward(s, e, k) : lane_backward(s, e, k);
}
template <bool WAVE>
__device__ __forceinline__ Range codepoint_range(const uint8_t* data, int64_t s_off, int64_t e_off, int64_t start, int64_t stop) {
  Range r{s_off, s_off};
  if (s_off == e_off) return r;          // (no referenced byte, and data may be NULL)
  const uint64_t d = reinterpret_cast<uint64_t>(data);
  const uint64_t s = d + static_cast<uint64_t>(s_off), e = d + static_cast<uint64_t>(e_off);
  const uint64_t end = stop == kNoStop ? e : codepoint_bound<WAVE>(s, e, stop);
  // a begin at or past `end` is `end` whatever it is, so a forward walk stops there.  start 0 walks too: a row that opens
  // with continuation bytes begins at its first lead
  uint64_t begin = start >= 0 ? codepoint_bound<WAVE>(s, end, start) : codepoint_bound<WAVE>(s, e, start);
  if (begin > end) begin = end;
  r.begin = static_cast<int64_t>(begin - d);
  r.end = static_cast<int64_t>(end - d);
  return r;
}

// ---------------------------------------------------------------- kernels
// binary_length: n + 1 offsets in, n lengths out.  A lane takes R = 16 / sizeof(O) consecutive rows: one 16-byte load of
// their offsets, the offset after them, one 16-byte store.
template <typename O>
__global__ __launch_bounds__(kBlock) void byte_length_kernel(Bits valid, const O* __restrict__ offsets, int64_t n, O* __restrict__ out) {
  constexpr int R = 16 / static_cast<int>(sizeof(O));
  const int64_t ngroups = (n + R - 1) / R;
  for (int64_t grp = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; grp < ngroups; grp += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t row0 = grp * R;
    const uint64_t ok = load_word(valid, row0 >> 6) >> (row0 & 63);   // (R divides 64: the lane's rows share a word)
    if (row0 + R <= n) {
      O o[R + 1], len[R];
      __builtin_memcpy(o, offsets + row0, 16);
      o[R] = offsets[row0 + R];
#pragma unroll
      for (int j = 0; j < R; ++j) len[j] = ((ok >> j) & 1) ? static_cast<O>(o[j + 1] - o[j]) : O{0};
      __builtin_memcpy(out + row0, len, 16);
    } else {
      for (int64_t r = row0; r < n; ++r) out[r] = ((ok >> (r - row0)) & 1) ? static_cast<O>(offsets[r + 1] - offsets[r]) : O{0};
    }
  }
}

// utf8_length, one lane per row
template <typename O>
__global__ __launch_bounds__(kBlock) void codepoint_length_rows_kernel(Bits valid, const O* __restrict__ offsets,
                                                                       const uint8_t* __restrict__ data, int64_t n, O* __restrict__ out) {
  const uint64_t d = reinterpret_cast<uint64_t>(data);
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; row < n; row += static_cast<int64_t>(gridDim.x) * kBlock) {
    const bool ok = (load_word(valid, row >> 6) >> (row & 63)) & 1;
    int64_t c = 0;
    if (ok) {
      const int64_t s_off = offsets[row], e_off = offsets[row + 1];
      if (e_off > s_off) c = lane_count(d + static_cast<uint64_t>(s_off), d + static_cast<uint64_t>(e_off));
    }
    out[row] = static_cast<O>(c);
  }
}

// utf8_length, one wave per row.  A wave takes 64 consecutive rows a step, one after the other; lane i keeps row i's
// count, so the step ends in one coalesced store.
template <typename O>
__global__ __launch_bounds__(kBlock) void codepoint_length_waves_kernel(Bits valid, const O* __restrict__ offsets,
                                                                        const uint8_t* __restrict__ data, int64_t n, O* __restrict__ out) {
  const uint64_t d = reinterpret_cast<uint64_t>(data);
  const int lane = lane_id();
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t base = wave * kWave; base < n; base += nwaves * kWave) {
    const uint64_t ok = load_word(valid, base >> 6);                // the step's 64 rows (0 past the end)
    int64_t mine = 0;
    for (int i = 0; i < kWave; ++i) {
      if (!((ok >> i) & 1)) continue;                               // (wave-uniform)
      const int64_t s_off = offsets[base + i], e_off = offsets[base + i + 1];
      if (e_off <= s_off) continue;
      const int64_t c = wave_count(d + static_cast<uint64_t>(s_off), d + static_cast<uint64_t>(e_off));
      if (lane == i) mine = c;
    }
    if (base + lane < n) out[base + lane] = static_cast<O>(mine);
  }
}

// step one of a slice, one lane per row: UNIT bytes or codepoints.  lens[row] = the output row's length, src[row] = the
// index of its first byte in data, sums[row / kBinRows] += the length (one atomic a wave: a wave's 64 rows share a sum)
template <typename O, int UNIT>
__global__ __launch_bounds__(kBlock) void slice_rows_kernel(Bits valid, const O* __restrict__ offsets, const uint8_t* __restrict__ data,
                                                            int64_t n, int64_t start, int64_t stop, O* __restrict__ lens,
                                                            O* __restrict__ src, unsigned long long* __restrict__ sums) {
  const int lane = lane_id();
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kBlock; base < n; base += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t row = base + threadIdx.x;
    const bool ok = (load_word(valid, row >> 6) >> lane) & 1;       // 0 past the end
    Range r{0, 0};
    if (row < n) {
      const int64_t s_off = offsets[row];
      r.begin = r.end = s_off;
      if (ok) {
        const int64_t e_off = offsets[row + 1];
        if constexpr (UNIT == ARX_STRING_UNIT_BYTES) r = byte_range(s_off, e_off, start, stop);
        else r = codepoint_range<false>(data, s_off, e_off, start, stop);
      }
      lens[row] = static_cast<O>(r.end - r.begin);
      src[row] = static_cast<O>(r.begin);
    }
    const uint64_t total = wave_reduce_sum_u64(static_cast<uint64_t>(r.end - r.begin));
    if (lane == 0 && total != 0) atomicAdd(&sums[(row - lane) / kBinRows], static_cast<unsigned long long>(total));
  }
}

// step one of a codepoint slice, one wave per row: 64 consecutive rows a step as above, so lens / src are stored
// coalesced and the step's bytes reach its sum in one atomic, as in the rows form
template <typename O>
__global__ __launch_bounds__(kBlock) void slice_waves_kernel(Bits valid, const O* __restrict__ offsets, const uint8_t* __restrict__ data,
                                                             int64_t n, int64_t start, int64_t stop, O* __restrict__ lens,
                                                             O* __restrict__ src, unsigned long long* __restrict__ sums) {
  const int lane = lane_id();
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t base = wave * kWave; base < n; base += nwaves * kWave) {
    const uint64_t ok = load_word(valid, base >> 6);                // the step's 64 rows (0 past the end)
    const int64_t row = base + lane;
    Range mine{0, 0};
    if (row < n) mine.begin = mine.end = offsets[row];
    for (int i = 0; i < kWave; ++i) {
      if (!((ok >> i) & 1)) continue;                               // (wave-uniform)
      const Range r = codepoint_range<true>(data, offsets[base + i], offsets[base + i + 1], start, stop);
      if (lane == i) mine = r;
    }
    if (row < n) {
      lens[row] = static_cast<O>(mine.end - mine.begin);
      src[row] = static_cast<O>(mine.begin);
    }
    const uint64_t total = wave_reduce_sum_u64(static_cast<uint64_t>(mine.end - mine.begin));
    if (lane == 0 && total != 0) atomicAdd(&sums[base / kBinRows], static_cast<unsigned long long>(total));
  }
}

template <typename O>
int length_launch(const Column& c, int unit, bool waves, void* out, hipStream_t st) {
  const O* offsets = static_cast<const O*>(c.offsets);
  if (unit == ARX_STRING_UNIT_BYTES) {
    const int64_t groups = ceil_div(c.n, 16 / static_cast<int64_t>(sizeof(O)));
    const unsigned grid = static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(ceil_div(groups, kBlock), kLengthMaxBlocks)));
    hipLaunchKernelGGL(byte_length_kernel<O>, dim3(grid), dim3(kBlock), 0, st, c.valid, offsets, c.n, static_cast<O*>(out));
    ARX_CHECK_LAUNCH("byte_length_kernel");
  } else if (waves) {
    hipLaunchKernelGGL(codepoint_length_waves_kernel<O>, dim3(waves_grid(c.n, kWave)), dim3(kBlock), 0, st, c.valid, offsets, c.data, c.n,
                       static_cast<O*>(out));
    ARX_CHECK_LAUNCH("codepoint_length_waves_kernel");
    g_slice_wave_launches.fetch_add(1, std::memory_order_relaxed);
  } else {
    hipLaunchKernelGGL(codepoint_length_rows_kernel<O>, dim3(rows_grid(c.n)), dim3(kBlock), 0, st, c.valid, offsets, c.data, c.n,
                       static_cast<O*>(out));
    ARX_CHECK_LAUNCH("codepoint_length_rows_kernel");
    g_slice_row_launches.fetch_add(1, std::memory_order_relaxed);
  }
  return ARX_OK;
}

// step one of a slice (the `produce` of offsets_call)
template <typename O>
int slice_offsets_launch(const Column& c, int unit, bool waves, int64_t start, int64_t stop, O* lens, O* src, unsigned long long* sums,
                         hipStream_t st) {
  const O* offsets = static_cast<const O*>(c.offsets);
  if (unit == ARX_STRING_UNIT_BYTES) {
    hipLaunchKernelGGL((slice_rows_kernel<O, ARX_STRING_UNIT_BYTES>), dim3(rows_grid(c.n)), dim3(kBlock), 0, st, c.valid, offsets, c.data,
                       c.n, start, stop, lens, src, sums);
    ARX_CHECK_LAUNCH("slice_rows_kernel (bytes)");
  } else if (waves) {
    hipLaunchKernelGGL(slice_waves_kernel<O>, dim3(waves_grid(c.n, kWave)), dim3(kBlock), 0, st, c.valid, offsets, c.data, c.n, start, stop,
                       lens, src, sums);
    ARX_CHECK_LAUNCH("slice_waves_kernel");
    g_slice_wave_launches.fetch_add(1, std::memory_order_relaxed);
  } else {
    hipLaunchKernelGGL((slice_rows_kernel<O, ARX_STRING_UNIT_CODEPOINTS>), dim3(rows_grid(c.n)), dim3(kBlock), 0, st, c.valid, offsets,
                       c.data, c.n, start, stop, lens, src, sums);
    ARX_CHECK_LAUNCH("slice_rows_kernel (codepoints)");
    g_slice_row_launches.fetch_add(1, std::memory_order_relaxed);
  }
  return ARX_OK;
}

int check_unit_path(const char* who, int unit, int path) {
  if (unit != ARX_STRING_UNIT_BYTES && unit != ARX_STRING_UNIT_CODEPOINTS) {
    set_error("%s: unit %d is not 0 (bytes) or 1 (codepoints)", who, unit);
    return ARX_INVALID;
  }
  return check_path(who, path);
}

}  // namespace

static const CounterRow kStringSliceCounters[] = {
    {"string_slice_row_launches", &g_slice_row_launches},
    {"string_slice_wave_launches", &g_slice_wave_launches},
};
CounterTable string_slice_counters() { return counter_table(kStringSliceCounters); }

}  // namespace arx

using namespace arx;

extern "C" {

int arx_string_length(const ArxBinarySpan* values, int offset_width, int unit, int64_t data_bytes_hint, int path, void* out_lengths,
                      void* stream) {
  if (values == nullptr || out_lengths == nullptr) {
    set_error("string_length: NULL values or out_lengths");
    return ARX_INVALID;
  }
  int rc = check_unit_path("string_length", unit, path);
  if (rc == ARX_OK) rc = check_common("string_length", values, offset_width);
  if (rc != ARX_OK) return rc;
  if (values->length == 0) return ARX_OK;
  if (values->offsets == nullptr) {
    set_error("string_length: NULL offsets of values");
    return ARX_INVALID;
  }
  const Column c = column_of(values, offset_width);
  const bool waves = take_waves(path, mean_bytes(data_bytes_hint, c.n));
  return with_offset_type(offset_width, [&](auto o) { return length_launch<decltype(o)>(c, unit, waves, out_lengths, as_stream(stream)); });
}

size_t arx_string_slice_workspace_bytes(int64_t length, int offset_width) {
  return bin_workspace_bytes(length, offset_width == 8 ? 8 : 4);
}

int arx_string_slice_offsets(const ArxBinarySpan* values, int offset_width, int unit, int64_t start, int64_t stop, int64_t data_bytes_hint,
                             int path, void* ws, size_t ws_bytes, void* out_offsets, int64_t* out_total_bytes, void* stream) {
  int rc = check_offsets_arguments("string_slice_offsets", values, out_offsets, out_total_bytes);
  if (rc == ARX_OK) rc = check_unit_path("string_slice_offsets", unit, path);
  if (rc != ARX_OK) return rc;
  return offsets_call("string_slice_offsets", "arx_string_slice_workspace_bytes", values, offset_width, ws, ws_bytes, out_offsets,
                      out_total_bytes, "slicing a binary array", as_stream(stream),
                      [&](const Column& c, auto* lens, auto* src, unsigned long long* sums, hipStream_t st) {
                        const bool waves = take_waves(path, mean_bytes(data_bytes_hint, c.n));
                        return slice_offsets_launch(c, unit, waves, start, stop, lens, src, sums, st);
                      });
}

int arx_string_slice_data(const ArxBinarySpan* values, int offset_width, const void* ws, size_t ws_bytes, const void* out_offsets,
                          int64_t total_bytes, void* out_data, void* stream) {
  if (values == nullptr) {
    set_error("string_slice_data: NULL values");
    return ARX_INVALID;
  }
  const int rc = check_common("string_slice_data", values, offset_width);
  if (rc != ARX_OK) return rc;
  if (total_bytes < 0) {
    set_error("string_slice_data: negative total_bytes %lld", static_cast<long long>(total_bytes));
    return ARX_INVALID;
  }
  const int64_t n = values->length;
  if (n == 0 || total_bytes == 0) return ARX_OK;
  if (out_offsets == nullptr || out_data == nullptr || values->data == nullptr) {
    set_error("string_slice_data: NULL out_offsets, out_data or data of values");
    return ARX_INVALID;
  }
  if (ws == nullptr || ws_bytes < bin_workspace_bytes(n, offset_width)) {
    set_error("string_slice_data: ws of %llu bytes is NULL or smaller than arx_string_slice_workspace_bytes = %llu (pass the workspace "
              "of the offsets call)", static_cast<unsigned long long>(ws_bytes),
              static_cast<unsigned long long>(bin_workspace_bytes(n, offset_width)));
    return ARX_INVALID;
  }
  const auto* data = static_cast<const uint8_t*>(values->data);
  const uint8_t* src = static_cast<const uint8_t*>(ws) + bin_sums_bytes(n);
  hipStream_t st = as_stream(stream);
  return with_offset_type(offset_width, [&](auto o) {
    using O = decltype(o);
    return bin_copy_rows<O>(data, reinterpret_cast<const O*>(src), static_cast<const O*>(out_offsets), n, total_bytes,
                            static_cast<uint8_t*>(out_data), 0, st);
  });
}

}  // extern "C"

// What the row-wise string kernels share (string_slice.hip, string_trim.hip, match_substring.hip, string_compare.hip,
// string_replace.hip).  Device side: the bit-7 byte masks of a 16-byte granule, the unaligned 8-byte read and the LDS
// staging of a literal operand, the window walk that finds a pattern's next match in a row.  Host side: the view of a
// values column, the grids of a one-lane-per-row and a one-wave-per-row launch, the choice between the two forms, the
// offset type of a call from its offset_width, the argument checks of the C entry points, and offsets_call: the frame of
// the first of the two calls that make a variable-length result (slices, trims, replace_substring), over offsets_frame,
// which serves a call of several operands (string_join.hip).
#pragma once
#include "binary_scan_copy.h"

#include <algorithm>
#include <atomic>

namespace arx {

constexpr uint64_t kBit7 = 0x8080808080808080ull;

// bit 7 of the bytes [from, to) of a 64-bit word, 0 <= from, to <= 8 after clamping
__device__ __forceinline__ uint64_t byte_range_bit7(int64_t from, int64_t to) {
  from = from < 0 ? 0 : from;
  to = to > 8 ? 8 : to;
  if (to <= from) return 0;
  const uint64_t below_to = to >= 8 ? ~uint64_t(0) : ((uint64_t(1) << (8 * to)) - 1);
  const uint64_t below_from = (uint64_t(1) << (8 * from)) - 1;   // from < 8 here
  return below_to & ~below_from & kBit7;
}

// up to 8 bytes at p (any alignment), of which the first `rem` >= 1 are referenced; the others read as zero.  One or
// two aligned words, the second only if it holds a referenced byte.
__device__ __forceinline__ uint64_t load_bytes8(const uint8_t* p, int64_t rem) {
  const uint64_t addr = reinterpret_cast<uint64_t>(p);
  const uint64_t* wp = reinterpret_cast<const uint64_t*>(addr & ~uint64_t(7));
  const int sh = static_cast<int>(addr & 7);
  uint64_t w = wp[0] >> (sh * 8);
  if (sh != 0 && (8 - sh) < rem) w |= wp[1] << (64 - sh * 8);
  if (rem < 8) w &= (uint64_t(1) << (8 * rem)) - 1;
  return w;
}

// A literal operand (the pattern of match_substring.hip, the scalar side of string_compare.hip, the pattern and the
// replacement of string_replace.hip): a device pointer.  Up to
// kPatternLdsCap bytes it is staged once per workgroup in LDS; a longer one is read where it lies (it stays in L2).
constexpr int kPatternLdsCap = 1024;
// the literal for this workgroup: staged in `s_pat` (zero-padded to whole words) when it fits, else where it lies
__device__ __forceinline__ const uint8_t* stage_pattern(uint64_t* s_pat, const uint8_t* g_pat, int64_t m) {
  if (m > kPatternLdsCap) return g_pat;
  const int words = static_cast<int>((m + 7) >> 3);
  for (int i = threadIdx.x; i < words; i += kBlock) s_pat[i] = load_bytes8(g_pat + 8 * i, m - 8 * i);
  __syncthreads();
  return reinterpret_cast<const uint8_t*>(s_pat);
}

// a[0, len) == b[0, len), len >= 0, every byte of both referenced
__device__ __forceinline__ bool bytes_equal(const uint8_t* a, const uint8_t* b, int64_t len) {
  for (int64_t k = 0; k < len; k += 8) {
    if (load_bytes8(a + k, len - k) != load_bytes8(b + k, len - k)) return false;
  }
  return true;
}

struct Prefix {
  uint64_t bytes, mask;   // the pattern's first min(m, 8) bytes and the mask of those bytes
};
__device__ __forceinline__ Prefix pattern_prefix(const uint8_t* pat, int64_t m) {
  Prefix p;
  p.mask = m >= 8 ? ~uint64_t(0) : ((uint64_t(1) << (8 * m)) - 1);
  p.bytes = load_bytes8(pat, m < 8 ? m : 8);
  return p;
}

// the first position p >= from at which row[p, p + m) == pat[0, m), or -1.  1 <= m, 0 <= from.  The lane walks the
// aligned 8-byte words of row[from, len) with a two-word sliding window: at every byte position one masked 64-bit compare
// tests the pattern's first min(m, 8) bytes, a hit verifies the remaining m - 8 bytes word by word.
__device__ __forceinline__ int64_t row_find(const uint8_t* row, int64_t len, const uint8_t* pat, int64_t m, Prefix pfx, int64_t from) {
  const int64_t last = len - m;          // the last start position
  if (from > last) return -1;
  const uint64_t addr = reinterpret_cast<uint64_t>(row) + static_cast<uint64_t>(from);
  const uint64_t end = reinterpret_cast<uint64_t>(row) + static_cast<uint64_t>(len);
  const uint64_t* wp = reinterpret_cast<const uint64_t*>(addr & ~uint64_t(7));
  int b = static_cast<int>(addr & 7);
  uint64_t cur = wp[0];
  for (int64_t p = from; p <= last;) {
    // the next word only if it holds a byte of the row
    const uint64_t next = reinterpret_cast<uint64_t>(wp + 1) < end ? wp[1] : 0;
    for (; b < 8 && p <= last; ++b, ++p) {
      const uint64_t win = b == 0 ? cur : ((cur >> (8 * b)) | (next << (64 - 8 * b)));
      if (((win ^ pfx.bytes) & pfx.mask) == 0 && (m <= 8 || bytes_equal(row + p + 8, pat + 8, m - 8))) return p;
    }
    b = 0;
    cur = next;
    ++wp;
  }
  return -1;
}

inline int device_cus() {
  static std::atomic<int> cus{0};
  int c = cus.load(std::memory_order_relaxed);
  if (c == 0) {
    int dev = 0, n = 0;
    c = (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
    cus.store(c, std::memory_order_relaxed);
  }
  return c;
}

// one lane per row, a workgroup strides over what is left
inline unsigned rows_grid(int64_t n) {
  return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, kBlock), static_cast<int64_t>(device_cus()) * 8)));
}

struct Column {
  Bits valid;
  const void* offsets;   // element 0 of the logical array
  const uint8_t* data;
  int64_t n;
};
inline Column column_of(const ArxBinarySpan* values, int offset_width) {
  Column c;
  c.n = values->length;
  c.offsets = reinterpret_cast<const uint8_t*>(values->offsets) + values->offset * offset_width;
  c.data = static_cast<const uint8_t*>(values->data);
  c.valid = make_bits(values->null_count == 0 ? nullptr : values->validity, values->offset, c.n);
  return c;
}

// one wave per row: a wave takes `chunk` consecutive rows a step (kWave in the slices and the comparisons, whose lane i
// keeps row i's result) and strides over what is left
inline unsigned waves_grid(int64_t n, int chunk = 1) {
  return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(ceil_div(ceil_div(n, chunk), kWavesPerBlock), static_cast<int64_t>(device_cus()) * 8)));
}

// The `path` of a call: 0 = auto, 1 = rows, 2 = waves, under the three public names of include/arrow_amd.h.
static_assert(ARX_STRING_PATH_AUTO == 0 && ARX_REPLACE_PATH_AUTO == 0 && ARX_COMPARE_PATH_AUTO == 0, "one auto");
static_assert(ARX_STRING_PATH_ROWS == 1 && ARX_REPLACE_PATH_ROWS == 1 && ARX_COMPARE_PATH_ROWS == 1, "one rows");
static_assert(ARX_STRING_PATH_WAVES == 2 && ARX_REPLACE_PATH_WAVES == 2 && ARX_COMPARE_PATH_WAVES == 2, "one waves");
inline int check_path(const char* who, int path) {
  if (path != ARX_STRING_PATH_AUTO && path != ARX_STRING_PATH_ROWS && path != ARX_STRING_PATH_WAVES) {
    set_error("%s: path %d is not 0 (auto), 1 (rows) or 2 (waves)", who, path);
    return ARX_INVALID;
  }
  return ARX_OK;
}
// auto: the waves form from this mean row size on.  Measured on the MI355X for the codepoint walk of the slices
// (scripts/exp_string_slice.py, profiles/string_slice.txt, both forms over 2^28 data bytes: counting a column, the rows
// form is ahead up to 128 bytes a row, 0.214 ms against 0.533 ms, the waves form from 512 on, 0.142 ms against 0.248 ms;
// a slice with small bounds reads a granule or two a row in either form and the rows form stays ahead, DESIGN.md 4.21 —
// the threshold bounds the other case, a bound deep inside long or skewed rows) and for replace_substring
// (scripts/exp_string_replace.py, profiles/string_replace.txt, 128 MiB of rows with a pattern that never occurs, both
// calls timed together: the rows form is ahead up to 256 bytes a row, 0.960 ms against 1.084 ms and 0.555 ms against
// 3.909 ms at 64, the waves form from 512 on, 0.589 ms against 0.907 ms and 0.284 ms against 1.692 ms at 4 KiB; a
// frequent pattern does not move it: at 64 bytes a row with two matches each the rows form takes 0.67 ms, the waves form
// 5.5 ms).
constexpr int64_t kWavesPathMeanRow = 512;
// the mean row size of a call from its data_bytes_hint (negative: unknown, and so is the mean); n > 0
inline int64_t mean_bytes(int64_t hint, int64_t n) { return hint < 0 ? -1 : hint / n; }
// the form of a call: on auto the waves form from the mean `from_mean` > 0 on, so never for an unknown (negative) mean
inline bool take_waves(int path, int64_t mean, int64_t from_mean = kWavesPathMeanRow) {
  return path == ARX_STRING_PATH_WAVES || (path == ARX_STRING_PATH_AUTO && mean >= from_mean);
}

// f(O{}) with O the offset type of a checked offset_width: int32_t for 4, int64_t for 8
template <typename F>
inline int with_offset_type(int offset_width, F&& f) {
  return offset_width == 4 ? f(int32_t{}) : f(int64_t{});
}

// the checks the calls share; `who` names the call
inline int check_common(const char* who, const ArxBinarySpan* values, int offset_width) {
  if (offset_width != 4 && offset_width != 8) {
    set_error("%s: offset_width %d is not 4 or 8", who, offset_width);
    return ARX_INVALID;
  }
  if (values->length < 0) {
    set_error("%s: negative length %lld of values", who, static_cast<long long>(values->length));
    return ARX_INVALID;
  }
  return ARX_OK;
}
// the workspace of an offsets call, [sums][src_start] of binary_scan_copy.h; `sizing` names the function that sizes it
inline int check_offsets_workspace(const char* who, const char* sizing, const void* ws, size_t ws_bytes, int64_t length, int offset_width) {
  if (ws == nullptr || ws_bytes < bin_workspace_bytes(length, offset_width) || (reinterpret_cast<uint64_t>(ws) & 7) != 0) {
    set_error("%s: ws of %llu bytes is NULL, unaligned or smaller than %s = %llu", who, static_cast<unsigned long long>(ws_bytes), sizing,
              static_cast<unsigned long long>(bin_workspace_bytes(length, offset_width)));
    return ARX_INVALID;
  }
  return ARX_OK;
}

// An OFFSETS CALL (arx_string_slice_offsets, arx_string_trim_offsets, arx_replace_substring_offsets): the first of the two
// calls that make a variable-length result out of the rows of `values`, one for one.  The entry point refuses its NULL
// arguments first (check_offsets_arguments) and runs its own checks, in its own order; offsets_call is all the rest.
//   length 0: *out_total_bytes = 0, out_offsets[0] = 0, nothing launched.
//   else: the workspace is carved (binary_scan_copy.h), its sums are zeroed, `produce(column, lens, src, sums, stream)`
//   launches the call's own first kernel under that header's contract (O* lens = out_offsets, O* src = the workspace's
//   second part, O the offset type) and counts the launch, and bin_scan_lengths turns the lengths into offsets and
//   returns the total: "offset overflow while <what>" where it does not fit.
// A refused call has written nothing.
inline int check_offsets_arguments(const char* who, const ArxBinarySpan* values, const void* out_offsets, const int64_t* out_total_bytes) {
  if (values == nullptr || out_offsets == nullptr || out_total_bytes == nullptr) {
    set_error("%s: NULL values, out_offsets or out_total_bytes", who);
    return ARX_INVALID;
  }
  return ARX_OK;
}
// offsets_frame is that rest for `length` rows of any number of operands (arx_binary_join_offsets has k + 1 of them, its
// own checks done): `produce(out, second, sums, stream)` with O* out = out_offsets and O* second = the workspace's second
// part.  lengths_in_ws: the producer keeps the lengths in `second` instead of out_offsets, which then stays untouched
// when the total is refused.
template <typename F>
int offsets_frame(const char* who, const char* sizing, int64_t length, int offset_width, void* ws, size_t ws_bytes, void* out_offsets,
                  int64_t* out_total_bytes, const char* what, bool lengths_in_ws, hipStream_t st, F&& produce) {
  if (length == 0) {
    *out_total_bytes = 0;
    ARX_HIP(hipMemsetAsync(out_offsets, 0, static_cast<size_t>(offset_width), st));
    return ARX_OK;
  }
  const int rc = check_offsets_workspace(who, sizing, ws, ws_bytes, length, offset_width);
  if (rc != ARX_OK) return rc;
  *out_total_bytes = 0;
  return with_offset_type(offset_width, [&](auto o) {
    using O = decltype(o);
    auto* sums = static_cast<unsigned long long*>(ws);
    O* second = reinterpret_cast<O*>(static_cast<uint8_t*>(ws) + bin_sums_bytes(length));
    O* out = static_cast<O*>(out_offsets);
    ARX_HIP(hipMemsetAsync(sums, 0, bin_sums_bytes(length), st));
    const int launched = produce(out, second, sums, st);
    if (launched != ARX_OK) return launched;
    return bin_scan_lengths<O>(out, length, reinterpret_cast<long long*>(sums), what, out_total_bytes, st, lengths_in_ws ? second : nullptr);
  });
}
template <typename F>
int offsets_call(const char* who, const char* sizing, const ArxBinarySpan* values, int offset_width, void* ws, size_t ws_bytes,
                 void* out_offsets, int64_t* out_total_bytes, const char* what, hipStream_t st, F&& produce) {
  const int rc = check_common(who, values, offset_width);   // (again, where the entry point's own checks ran it in their place)
  if (rc != ARX_OK) return rc;
  if (values->length > 0 && values->offsets == nullptr) {
    set_error("%s: NULL offsets of values", who);
    return ARX_INVALID;
  }
  const Column c = column_of(values, offset_width);
  return offsets_frame(who, sizing, c.n, offset_width, ws, ws_bytes, out_offsets, out_total_bytes, what, false, st,
                       [&](auto* lens, auto* src, unsigned long long* sums, hipStream_t s) { return produce(c, lens, src, sums, s); });
}

}  // namespace arx

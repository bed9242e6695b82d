// Substring predicates on utf8 / binary columns and their large forms: match_substring, starts_with, ends_with with a
// literal pattern — the reference's PlainSubstringMatcher / PlainStartsWithMatcher / PlainEndsWithMatcher
// (compute/kernels/scalar_string_ascii.cc) with ignore_case = false.  Bytes compare as bytes: no UTF-8 awareness, a
// '\0' is an ordinary byte.  The output is a bitmap at offset 0 (bit i = row i matches, 0 for a null row); the
// validity of the result is the input's and is the caller's copy (arx_bitmap_copy).
//
// Two kernels.
//   rows  (all three functions): one lane per row, 64 rows = one __ballot word written whole by lane 0.  The lane walks
//         the aligned 8-byte words of its row with a two-word sliding window; at every byte position one masked 64-bit
//         compare tests the pattern's first min(m, 8) bytes, a hit verifies the remaining m - 8 bytes word by word.
//         starts_with / ends_with compare m bytes at the head / tail and skip rows shorter than m.
//   bytes (match_substring): a lane with a long row would hold the whole row while 63 lanes idle and neighbours read far
//         apart, so this kernel walks the BYTES: a persistent grid reads offsets[0] and offsets[length] itself and splits
//         the tiles (256 aligned 16-byte granules each) of the referenced range data[offsets[0], offsets[length])
//         into one contiguous run per workgroup; a lane tests the 16 start positions of its granule
//         (the same masked compare, then the verify), finds the row that owns a hit by binary search inside the tile's
//         row range (offsets staged in LDS when they fit), accepts it if the match ends inside that row and the row is
//         valid, and ORs the row's bit into the zeroed output.
//
// Pattern: a device pointer.  Up to kPatternLdsCap bytes (string_rows.h) it is staged once per workgroup in LDS; a
// longer one is read where it lies through the same pointer variable (it stays in L2).  1 KiB holds every literal a filter is written
// with and costs a workgroup 1/160 of the CU's LDS, no occupancy.
//
// Granule rule: a load touches only an aligned 8- or 16-byte piece that holds at least one referenced byte (of the row
// in the rows kernel, of data[offsets[0], offsets[length]) in the bytes kernel, of the pattern for pattern reads), so
// nothing is read before the 16-byte granule of the first referenced byte or past the granule of the last one.
//
// Worst case: no KMP / two-way table.  A hit of the 8-byte prefix starts a verify that restarts at the next position, so
// a pattern a^k b against rows of a's costs O(row bytes x m) — quadratic in the adversarial case, linear for text.
#include "string_rows.h"

namespace arx {

namespace {

constexpr int kGranule = 16;               // bytes a lane of the bytes kernel owns
constexpr int kTileBytes = kBlock * kGranule;   // 4 KiB of data per workgroup step
constexpr int kStageOffsets = 2048;        // offsets of a tile's row range staged in LDS (a 4 KiB tile of >= 2-byte rows)
constexpr int kByteGroupsPerCU = 8;        // persistent grid of the bytes kernel: the 8 workgroups of 256 a CU holds (8 x 17 KiB of LDS)
// auto (path 0): the bytes kernel from this mean row size (data_bytes_hint / length) on.  Measured on the MI355X
// (scripts/exp_match_substring.py, profiles/match_substring.txt, the sweep of the mean row size over 128 MiB with a rare
// pattern): the rows kernel is ahead up to 64 bytes (0.167 ms against 0.221 ms), the bytes kernel from 128 bytes on
// (0.191 ms against 0.230 ms; 0.157 ms against 1.124 ms at 4 KiB).  A frequent pattern favours the rows kernel at any
// size, since a lane stops at its row's first match — the threshold bounds the worst case instead:
// the rows kernel on a skewed column is 350 x behind, the bytes kernel on a frequent pattern 21 x.
constexpr int64_t kBytesPathMeanRow = 128;

std::atomic<int64_t> g_match_row_launches{0}, g_match_byte_launches{0};

// does row[0, len) contain pat[0, m)?  1 <= m <= len.  (the window walk: row_find of string_rows.h)
__device__ __forceinline__ bool row_contains(const uint8_t* row, int64_t len, const uint8_t* pat, int64_t m, Prefix pfx) {
  return row_find(row, len, pat, m, pfx, 0) >= 0;
}

// ---------------------------------------------------------------- rows
template <typename O>
__global__ __launch_bounds__(kBlock) void match_rows_kernel(Bits valid, const O* __restrict__ offsets, const uint8_t* __restrict__ data,
                                                            int64_t n, int op, const uint8_t* __restrict__ g_pat, int64_t m,
                                                            uint64_t* __restrict__ out_bits) {
  __shared__ uint64_t s_pat[kPatternLdsCap / 8];
  const uint8_t* pat = g_pat;
  Prefix pfx{0, 0};
  if (m > 0) {
    pat = stage_pattern(s_pat, g_pat, m);
    pfx = pattern_prefix(pat, m);
  }
  const int lane = lane_id();
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kBlock; base < n; base += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t row = base + threadIdx.x;
    const bool ok = (load_word(valid, row >> 6) >> lane) & 1;   // 0 past the end
    bool hit = ok;                                              // the empty pattern: every valid row
    if (ok && m > 0) {
      const int64_t start = offsets[row];
      const int64_t len = static_cast<int64_t>(offsets[row + 1]) - start;
      hit = false;
      if (len >= m) {
        const uint8_t* r = data + start;
        if (op == ARX_MATCH_SUBSTRING) {
          hit = row_contains(r, len, pat, m, pfx);
        } else {
          hit = bytes_equal(op == ARX_MATCH_STARTS_WITH ? r : r + (len - m), pat, m);
        }
      }
    }
    const uint64_t word = __ballot(hit);
    if (row < n && lane == 0) out_bits[row >> 6] = word;
  }
}

// ---------------------------------------------------------------- bytes
// the largest k in [0, count) with off[k] <= p (off[0] <= p is given)
template <typename O>
__device__ __forceinline__ int64_t last_not_above(const O* off, int64_t count, int64_t p) {
  int64_t lo = 0, hi = count;   // off[lo] <= p, and off[hi] > p or hi == count
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (static_cast<int64_t>(off[mid]) <= p) lo = mid; else hi = mid;
  }
  return lo;
}

template <typename O>
__global__ __launch_bounds__(kBlock) void match_bytes_kernel(Bits valid, const O* __restrict__ offsets, const uint8_t* __restrict__ data,
                                                             int64_t n, const uint8_t* __restrict__ g_pat, int64_t m,
                                                             unsigned long long* __restrict__ out_bits) {
  __shared__ uint64_t s_pat[kPatternLdsCap / 8];
  __shared__ O s_off[kStageOffsets];
  __shared__ int64_t s_row;
  __shared__ int s_cnt[2];
  const uint8_t* pat = stage_pattern(s_pat, g_pat, m);
  const Prefix pfx = pattern_prefix(pat, m);
  const int64_t b0 = offsets[0], b1 = offsets[n];          // the referenced bytes data[b0, b1)
  if (b1 - b0 < m) return;                                  // (uniform: no row can hold the pattern)
  const uint64_t d = reinterpret_cast<uint64_t>(data);
  const uint64_t g_first = (d + static_cast<uint64_t>(b0)) >> 4, g_last = (d + static_cast<uint64_t>(b1) - 1) >> 4;
  const int64_t tiles = static_cast<int64_t>((g_last - g_first) / kBlock) + 1;
  // a workgroup takes a contiguous run of tiles, so that the row owning a tile's last byte is where the next tile's
  // rows start: one full binary search per workgroup, then the upper end of each tile's row range comes out of the
  // staging pass itself (one round of coalesced offset loads) instead of ~log2(length) dependent loads per 4 KiB
  const int64_t per = (tiles + gridDim.x - 1) / gridDim.x;
  const int64_t t_begin = static_cast<int64_t>(blockIdx.x) * per, t_end = std::min<int64_t>(tiles, t_begin + per);
  if (t_begin >= t_end) return;                             // (uniform)
  if (threadIdx.x == 0) {
    const int64_t p = std::max<int64_t>(b0, static_cast<int64_t>(((g_first + static_cast<uint64_t>(t_begin) * kBlock) << 4) - d));
    s_row = last_not_above(offsets, n + 1, p);
    s_cnt[0] = s_cnt[1] = 0;
  }
  __syncthreads();
  int64_t r_lo = s_row;                                     // offsets[r_lo] <= the tile's first referenced byte
  const int lane = lane_id();
  for (int64_t t = t_begin; t < t_end; ++t) {
    const uint64_t g_tile = g_first + static_cast<uint64_t>(t) * kBlock;
    const uint64_t g_end = std::min<uint64_t>(g_tile + kBlock - 1, g_last);
    const int64_t p_last = std::min<int64_t>(b1 - 1, static_cast<int64_t>((g_end << 4) + 15 - d));   // the tile's last referenced byte
    // stage the offsets from r_lo on and count those <= p_last (a prefix: offsets ascend): rows r_lo .. r_lo + count - 1
    // own the tile's bytes, the row of the last byte included
    __syncthreads();                                        // (the previous tile's readers of s_off / s_row are done)
    const int64_t avail = std::min<int64_t>(kStageOffsets, n + 1 - r_lo);
    int c = 0;
    for (int64_t i = threadIdx.x; i < avail; i += kBlock) {
      const O v = offsets[r_lo + i];
      s_off[i] = v;
      c += static_cast<int64_t>(v) <= p_last ? 1 : 0;
    }
    if (c != 0) atomicAdd(&s_cnt[t & 1], c);
    __syncthreads();
    int64_t r_count = s_cnt[t & 1];
    if (threadIdx.x == 0) s_cnt[(t + 1) & 1] = 0;
    const bool staged = r_count < avail;                    // the offset that ends the last row is staged too
    if (!staged) {                                          // (uniform) more rows than the stage holds: search on in global
      if (threadIdx.x == 0) {
        const int64_t from = r_lo + avail - 1;
        s_row = from + last_not_above(offsets + from, n + 1 - from, p_last);
      }
      __syncthreads();
      r_count = s_row - r_lo + 1;
    }
    const O* off = staged ? s_off : offsets + r_lo;

    const uint64_t g = g_tile + threadIdx.x;
    const bool active = g <= g_last;
    uint64_t lo = 0, hi = 0;
    if (active) {
      const uint4 q = *reinterpret_cast<const uint4*>(g << 4);
      lo = q.x | (static_cast<uint64_t>(q.y) << 32);
      hi = q.z | (static_cast<uint64_t>(q.w) << 32);
    }
    // the 8 bytes after the granule: the next lane's, or a load of the next granule if that holds a referenced byte
    uint64_t after = __shfl_down(lo, 1, 64);
    if (lane == 63) after = (active && g + 1 <= g_last) ? *reinterpret_cast<const uint64_t*>((g + 1) << 4) : 0;
    const int64_t p0 = static_cast<int64_t>((g << 4) - d);  // the granule's first byte as an index into data (may be < b0)
    int64_t c_row = -1, c_start = 0, c_end = 0;             // the row of this lane's previous hit
    for (int j = 0; active && j < kGranule; ++j) {
      const int64_t p = p0 + j;
      if (p < b0 || p + m > b1) continue;
      uint64_t win;
      if (j == 0) win = lo;
      else if (j < 8) win = (lo >> (8 * j)) | (hi << (64 - 8 * j));
      else if (j == 8) win = hi;
      else win = (hi >> (8 * (j - 8))) | (after << (64 - 8 * (j - 8)));
      if (((win ^ pfx.bytes) & pfx.mask) != 0) continue;
      if (m > 8 && !bytes_equal(data + p + 8, pat + 8, m - 8)) continue;
      if (c_row < 0 || p < c_start || p >= c_end) {
        const int64_t k = last_not_above(off, r_count, p);  // empty rows share their offset with the owner: the last one wins
        c_row = r_lo + k;
        c_start = off[k];
        c_end = off[k + 1];
      }
      if (p + m > c_end) continue;                          // a match may not span two rows
      if (!((load_word(valid, c_row >> 6) >> (c_row & 63)) & 1)) continue;
      unsigned long long* w = out_bits + (c_row >> 6);
      const unsigned long long bit = 1ull << (c_row & 63);
      if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(w, bit);
    }
    r_lo += r_count - 1;                                    // the row of this tile's last byte may go on in the next tile
  }
}

template <typename O>
int match_launch(const ArxBinarySpan* values, int op, const uint8_t* pat, int64_t m, int64_t hint, bool bytes, void* out_bits,
                 hipStream_t st) {
  const int64_t n = values->length;
  const O* offsets = reinterpret_cast<const O*>(values->offsets) + values->offset;
  const auto* data = static_cast<const uint8_t*>(values->data);
  const Bits valid = make_bits(values->null_count == 0 ? nullptr : values->validity, values->offset, n);
  if (bytes) {
    ARX_HIP(hipMemsetAsync(out_bits, 0, static_cast<size_t>((n + 63) / 64) * 8, st));
    const int64_t cap = static_cast<int64_t>(device_cus()) * kByteGroupsPerCU;
    const int64_t grid = hint < 0 ? cap : std::max<int64_t>(1, std::min<int64_t>(hint / kTileBytes + 2, cap));
    hipLaunchKernelGGL(match_bytes_kernel<O>, dim3(static_cast<unsigned>(grid)), dim3(kBlock), 0, st, valid, offsets, data, n, pat, m,
                       static_cast<unsigned long long*>(out_bits));
    ARX_CHECK_LAUNCH("match_bytes_kernel");
    g_match_byte_launches.fetch_add(1, std::memory_order_relaxed);
  } else {
    const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, static_cast<int64_t>(device_cus()) * 8));
    hipLaunchKernelGGL(match_rows_kernel<O>, dim3(static_cast<unsigned>(grid)), dim3(kBlock), 0, st, valid, offsets, data, n, op, pat, m,
                       static_cast<uint64_t*>(out_bits));
    ARX_CHECK_LAUNCH("match_rows_kernel");
    g_match_row_launches.fetch_add(1, std::memory_order_relaxed);
  }
  return ARX_OK;
}

}  // namespace

static const CounterRow kMatchSubstringCounters[] = {
    {"match_substring_row_launches", &g_match_row_launches},
    {"match_substring_byte_launches", &g_match_byte_launches},
};
CounterTable match_substring_counters() { return counter_table(kMatchSubstringCounters); }

}  // namespace arx

using namespace arx;

extern "C" {

int arx_match_substring(const ArxBinarySpan* values, int offset_width, int op, const void* pattern, int64_t pattern_length,
                        int64_t data_bytes_hint, int path, void* out_bits, void* stream) {
  if (values == nullptr || out_bits == nullptr) {
    set_error("match_substring: NULL values or out_bits");
    return ARX_INVALID;
  }
  if (op != ARX_MATCH_SUBSTRING && op != ARX_MATCH_STARTS_WITH && op != ARX_MATCH_ENDS_WITH) {
    set_error("match_substring: op %d is not 0 (match_substring), 1 (starts_with) or 2 (ends_with)", op);
    return ARX_INVALID;
  }
  if (path != ARX_MATCH_PATH_AUTO && path != ARX_MATCH_PATH_ROWS && path != ARX_MATCH_PATH_BYTES) {
    set_error("match_substring: path %d is not 0 (auto), 1 (rows) or 2 (bytes)", path);
    return ARX_INVALID;
  }
  if (offset_width != 4 && offset_width != 8) {
    set_error("match_substring: offset_width %d is not 4 or 8", offset_width);
    return ARX_INVALID;
  }
  if (values->length < 0 || pattern_length < 0) {
    set_error("match_substring: negative length (values %lld, pattern %lld)", static_cast<long long>(values->length),
              static_cast<long long>(pattern_length));
    return ARX_INVALID;
  }
  if (values->length == 0) return ARX_OK;
  if (values->offsets == nullptr || (pattern_length > 0 && pattern == nullptr)) {
    set_error("match_substring: NULL offsets or pattern");
    return ARX_INVALID;
  }
  // the bytes kernel is match_substring's alone, and never sees the empty pattern (every valid row: the rows kernel)
  bool bytes = false;
  if (op == ARX_MATCH_SUBSTRING && pattern_length > 0) {
    bytes = path == ARX_MATCH_PATH_BYTES ||
            (path == ARX_MATCH_PATH_AUTO && data_bytes_hint >= 0 && data_bytes_hint / values->length >= kBytesPathMeanRow);
  }
  const auto* pat = static_cast<const uint8_t*>(pattern);
  return with_offset_type(offset_width, [&](auto o) {
    return match_launch<decltype(o)>(values, op, pat, pattern_length, data_bytes_hint, bytes, out_bits, as_stream(stream));
  });
}

}  // extern "C"

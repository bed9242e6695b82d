// replace_substring on utf8 / binary columns and their large forms: the reference's PlainSubstringReplacer
// (compute/kernels/scalar_string_ascii.cc) under ReplaceSubstringOptions{pattern, replacement, max_replacements}.  Bytes
// are bytes: no UTF-8 awareness, '\0' and 0xff are ordinary bytes.  The first string kernel here whose output row is
// ASSEMBLED ("gap, replacement, gap, ...") instead of being a sub-range of its input row.
//
// Matches are found left to right and do not overlap: after a match at p the search resumes at p + m, the replacement is
// never re-scanned, and a match lies wholly inside its row.  max_replacements < 0: unlimited; 0: the rows unchanged;
// k > 0: the first k matches of each row.  The empty pattern has no kernel (the reference loops forever on it).
//
// Two calls, since the output size depends on the data (binary_scan_copy.h):
//   arx_replace_substring_offsets  counts each valid row's accepted matches c into the workspace, writes the output
//       row's length len + c (r - m) (64-bit arithmetic) into out_offsets, adds the lengths of every kBinRows rows into
//       the workspace's 64-bit sums (one atomic a wave), scans (bin_scan_lengths) and returns the total;
//   arx_replace_substring_data     walks the rows again and writes them; a row with c = 0 is a plain copy and is not
//       searched a second time.
// Workspace: [sums][c of every row, offset_width bytes each] — the layout and size of the slices' workspace.
//
// Two forms.
//   rows  : one lane per row.  The lane walks its row with the sliding two-word window of string_rows.h (row_find),
//           resuming behind every match; the writing pass copies 8 bytes a step (aligned loads, unaligned stores).
//   waves : one wave per row, for long or skewed rows.  In the counting pass a wave takes 1 .. 64 consecutive rows a step
//           (waves_chunk: as few as still fill the grid — the slices' fixed 64 left two waves a CU with work on 32768 rows
//           of 4 KiB) and lane i keeps row i's length and count, so they are stored coalesced and a sum gets one atomic
//           a step (one atomic a row: 131072 rows add to 32 sums and the atomics on one address take longer than the
//           rows).  In the writing pass the waves of the grid stride over the rows.  A step of a row is one tile of 64 aligned 16-byte granules (1 KiB): a lane tests the start positions of its granule (the same
//           masked compare, then the verify); candidates are accepted in position order by ballot while q >= next_free and
//           the cap allows, and next_free carries over from tile to tile, so a match may straddle tiles.  The writing
//           pass repeats the acceptance with the row's count as the cap and places each lane's bytes at
//           row_out + (src - row_start) + accepted_before x (r - m): stores of consecutive lanes are consecutive, and a
//           granule no match touches is one 16-byte store.
//
// Pattern and replacement: device pointers.  Up to kPatternLdsCap bytes (string_rows.h) each is staged once per
// workgroup in LDS; a longer one is read where it lies.
//
// Granule rule (as match_substring.hip): a load touches only an aligned 8- or 16-byte piece that holds at least one
// referenced byte of a valid row, or of the literal.  A null row's bytes are never read, whatever its offsets span.
//
// Worst case: as match_substring.hip, no KMP table — a^k b against rows of a's costs O(row bytes x m).  The waves form
// accepts one match per ballot round: a tile that is nothing but matches of a 2-byte pattern takes 512 rounds (a 1-byte
// pattern cannot overlap itself and is accepted with one popcount).
#include "string_rows.h"

namespace arx {

namespace {

constexpr int kGranule = 16;                     // bytes a lane of the waves form owns a step
constexpr int kTileBytes = kWave * kGranule;     // 1 KiB of a row per wave step
constexpr int64_t kNoCap = INT64_MAX;
// auto (path 0): the waves form from a mean row size of kWavesPathMeanRow on (string_rows.h).  The offsets call:
// data_bytes_hint / length; the data call, which is handed no hint: total_bytes / length, the bytes it writes a row.

std::atomic<int64_t> g_replace_row_launches{0}, g_replace_wave_launches{0};

struct Literals {
  const uint8_t* pat;   // m >= 1 bytes
  int64_t m;
  Prefix pfx;
  const uint8_t* rep;   // r >= 0 bytes
  int64_t r;
};

// dst[0, len) = src[0, len): src is read in aligned words that hold a byte of it, dst takes any alignment
__device__ __forceinline__ void lane_copy(uint8_t* dst, const uint8_t* src, int64_t len) {
  int64_t k = 0;
  for (; k + 8 <= len; k += 8) {
    const uint64_t w = load_bytes8(src + k, 8);
    __builtin_memcpy(dst + k, &w, 8);
  }
  if (k < len) {
    uint64_t w = load_bytes8(src + k, len - k);
    for (; k < len; ++k, w >>= 8) dst[k] = static_cast<uint8_t>(w);
  }
}

// ---------------------------------------------------------------- one lane per row
// the accepted matches of row[0, len), at most cap
__device__ __forceinline__ int64_t lane_count_matches(const uint8_t* row, int64_t len, const Literals& l, int64_t cap) {
  int64_t c = 0;
  for (int64_t p = 0; c < cap;) {
    const int64_t q = row_find(row, len, l.pat, l.m, l.pfx, p);
    if (q < 0) break;
    ++c;
    p = q + l.m;
  }
  return c;
}

// step one: lens[row] = the output row's length, cnt[row] = its accepted matches, sums[row / kBinRows] += the length
template <typename O>
__global__ __launch_bounds__(kBlock) void replace_count_rows_kernel(Bits valid, const O* __restrict__ offsets, const uint8_t* __restrict__ data,
                                                                    int64_t n, const uint8_t* __restrict__ g_pat, int64_t m, int64_t r,
                                                                    int64_t cap, O* __restrict__ lens, O* __restrict__ cnt,
                                                                    unsigned long long* __restrict__ sums) {
  __shared__ uint64_t s_pat[kPatternLdsCap / 8];
  Literals l;
  l.pat = stage_pattern(s_pat, g_pat, m);
  l.m = m;
  l.pfx = pattern_prefix(l.pat, m);
  l.rep = nullptr;
  l.r = r;
  const int lane = lane_id();
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kBlock; base < n; base += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t row = base + threadIdx.x;
    const bool ok = (load_word(valid, row >> 6) >> lane) & 1;       // 0 past the end
    int64_t out_len = 0, c = 0;
    if (ok) {
      const int64_t start = offsets[row];
      const int64_t len = static_cast<int64_t>(offsets[row + 1]) - start;
      if (cap != 0 && len >= m) c = lane_count_matches(data + start, len, l, cap);
      out_len = len + c * (r - m);
    }
    if (row < n) {
      lens[row] = static_cast<O>(out_len);
      cnt[row] = static_cast<O>(c);
    }
    const uint64_t total = wave_reduce_sum_u64(static_cast<uint64_t>(out_len));
    if (lane == 0 && total != 0) atomicAdd(&sums[(row - lane) / kBinRows], static_cast<unsigned long long>(total));
  }
}

// step two: "gap, replacement, gap, ..." of every valid row at out + out_offsets[row]
template <typename O>
__global__ __launch_bounds__(kBlock) void replace_write_rows_kernel(Bits valid, const O* __restrict__ offsets, const uint8_t* __restrict__ data,
                                                                    int64_t n, const uint8_t* __restrict__ g_pat, int64_t m,
                                                                    const uint8_t* __restrict__ g_rep, int64_t r, const O* __restrict__ cnt,
                                                                    const O* __restrict__ out_offsets, uint8_t* __restrict__ out) {
  __shared__ uint64_t s_pat[kPatternLdsCap / 8];
  __shared__ uint64_t s_rep[kPatternLdsCap / 8];
  Literals l;
  l.pat = stage_pattern(s_pat, g_pat, m);
  l.m = m;
  l.pfx = pattern_prefix(l.pat, m);
  l.rep = stage_pattern(s_rep, g_rep, r);
  l.r = r;
  for (int64_t row = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; row < n; row += static_cast<int64_t>(gridDim.x) * kBlock) {
    if (!((load_word(valid, row >> 6) >> (row & 63)) & 1)) continue;
    const int64_t start = offsets[row];
    const int64_t len = static_cast<int64_t>(offsets[row + 1]) - start;
    const uint8_t* src = data + start;
    uint8_t* dst = out + static_cast<int64_t>(out_offsets[row]);
    const int64_t c = cnt[row];
    int64_t p = 0;
    for (int64_t k = 0; k < c; ++k) {
      const int64_t q = row_find(src, len, l.pat, m, l.pfx, p);
      if (q < 0) break;                                             // (the count pass found c of them)
      lane_copy(dst, src + p, q - p);
      dst += q - p;
      lane_copy(dst, l.rep, r);
      dst += r;
      p = q + m;
    }
    lane_copy(dst, src + p, len - p);
  }
}

// ---------------------------------------------------------------- one wave per row
// What a lane knows of its granule g = tile + 16 lane after the tile's acceptance.
struct LaneHits {
  uint64_t lo, hi;    // the granule's bytes (0 for a lane past the row's end)
  uint32_t acc;       // bit j: an accepted match starts at g + j
  int64_t before;     // accepted matches of the row that start before g
  uint64_t cover;     // the end (address) of the last accepted match that starts before g: bytes below it are replaced
};

// bit j set: j < k (k any sign)
__device__ __forceinline__ uint32_t low_bits16(int64_t k) { return k <= 0 ? 0u : (k >= 16 ? 0xFFFFu : ((1u << k) - 1)); }

// One tile of the row [s, e) (addresses; s, e, tile, cap, count, next_free wave-uniform; all 64 lanes call).  search: test
// the tile's start positions and accept in position order while q >= next_free and count < cap; else the lanes only load
// their granules.  count and next_free carry over to the next tile.
__device__ __forceinline__ LaneHits wave_tile(uint64_t s, uint64_t e, uint64_t tile, const Literals& l, int64_t cap, bool search,
                                              int64_t& count, uint64_t& next_free) {
  const int lane = lane_id();
  const uint64_t g = tile + static_cast<uint64_t>(kGranule) * lane;
  const bool active = g < e;                                        // (g + 16 > s: the first tile starts at s's granule)
  LaneHits h;
  h.lo = h.hi = 0;
  h.acc = 0;
  h.before = count;
  h.cover = next_free;
  if (active) {
    const uint4 q = *reinterpret_cast<const uint4*>(g);
    h.lo = q.x | (static_cast<uint64_t>(q.y) << 32);
    h.hi = q.z | (static_cast<uint64_t>(q.w) << 32);
  }
  if (!search) return h;                                            // (uniform)
  // the 8 bytes after the granule: the next lane's, or a load of the next tile's first word if it holds a byte of the row
  uint64_t after = __shfl_down(h.lo, 1, 64);
  if (lane == 63) after = (active && g + kGranule < e) ? *reinterpret_cast<const uint64_t*>(g + kGranule) : 0;
  uint32_t cand = 0;
  for (int j = 0; active && j < kGranule; ++j) {
    const uint64_t a = g + j;
    if (a < s || a + static_cast<uint64_t>(l.m) > e) continue;
    uint64_t win;
    if (j == 0) win = h.lo;
    else if (j < 8) win = (h.lo >> (8 * j)) | (h.hi << (64 - 8 * j));
    else if (j == 8) win = h.hi;
    else win = (h.hi >> (8 * (j - 8))) | (after << (64 - 8 * (j - 8)));
    if (((win ^ l.pfx.bytes) & l.pfx.mask) != 0) continue;
    if (l.m > 8 && !bytes_equal(reinterpret_cast<const uint8_t*>(a) + 8, l.pat + 8, l.m - 8)) continue;
    cand |= 1u << j;
  }
  if (l.m == 1) {
    // a 1-byte pattern does not overlap itself: every candidate is accepted, unless the cap falls inside this tile
    const uint32_t mine = static_cast<uint32_t>(__popc(cand));
    const uint32_t incl = wave_inclusive_scan_u32(mine);
    const int64_t total = __shfl(incl, 63, 64);
    if (total <= cap - count) {                                     // (uniform)
      h.acc = cand;
      h.before = count + (incl - mine);
      count += total;
      return h;
    }
  }
  uint32_t rem = cand & ~low_bits16(static_cast<int64_t>(next_free - g));
  while (count < cap) {
    const uint64_t holders = __ballot(rem != 0);
    if (holders == 0) break;
    const int first = __ffsll(static_cast<unsigned long long>(holders)) - 1;
    const int j = __shfl(__ffsll(static_cast<unsigned long long>(rem)) - 1, first, 64);
    const uint64_t q = tile + static_cast<uint64_t>(kGranule) * first + j;
    if (lane == first) h.acc |= 1u << j;
    next_free = q + static_cast<uint64_t>(l.m);
    ++count;
    if (lane > first) {
      ++h.before;
      h.cover = next_free;
    }
    rem &= ~low_bits16(static_cast<int64_t>(next_free - g));
  }
  return h;
}

// the accepted matches of the row [s, e), at most cap; e - s >= m
__device__ __forceinline__ int64_t wave_count_matches(uint64_t s, uint64_t e, const Literals& l, int64_t cap) {
  int64_t count = 0;
  uint64_t next_free = s;
  for (uint64_t tile = s & ~uint64_t(kGranule - 1); tile < e && count < cap; tile += kTileBytes) wave_tile(s, e, tile, l, cap, true, count, next_free);
  return count;
}

// the output of the row [s, e) with c accepted matches at `dst`
__device__ __forceinline__ void wave_write_row(uint64_t s, uint64_t e, const Literals& l, int64_t c, uint8_t* dst) {
  const int lane = lane_id();
  const int64_t delta = l.r - l.m;
  int64_t count = 0;
  uint64_t next_free = s;
  for (uint64_t tile = s & ~uint64_t(kGranule - 1); tile < e; tile += kTileBytes) {
    const LaneHits h = wave_tile(s, e, tile, l, c, count < c, count, next_free);
    const uint64_t g = tile + static_cast<uint64_t>(kGranule) * lane;
    if (g >= e) continue;
    if (h.acc == 0 && h.cover <= g && g >= s && g + kGranule <= e) {
      // a whole granule no match touches: one store
      const uint4 q = make_uint4(static_cast<uint32_t>(h.lo), static_cast<uint32_t>(h.lo >> 32), static_cast<uint32_t>(h.hi),
                                 static_cast<uint32_t>(h.hi >> 32));
      __builtin_memcpy(dst + static_cast<int64_t>(g - s) + h.before * delta, &q, 16);
      continue;
    }
    int64_t k = h.before;
    uint64_t cover = h.cover;
    for (int j = 0; j < kGranule; ++j) {
      const uint64_t a = g + j;
      if (a < s || a >= e || a < cover) continue;
      uint8_t* at = dst + static_cast<int64_t>(a - s) + k * delta;
      if ((h.acc >> j) & 1) {
        lane_copy(at, l.rep, l.r);
        cover = a + static_cast<uint64_t>(l.m);
        ++k;
      } else {
        *at = static_cast<uint8_t>((j < 8 ? h.lo >> (8 * j) : h.hi >> (8 * (j - 8))) & 0xFF);
      }
    }
  }
}

template <typename O>
__global__ __launch_bounds__(kBlock) void replace_count_waves_kernel(Bits valid, const O* __restrict__ offsets, const uint8_t* __restrict__ data,
                                                                     int64_t n, const uint8_t* __restrict__ g_pat, int64_t m, int64_t r,
                                                                     int64_t cap, int chunk, O* __restrict__ lens, O* __restrict__ cnt,
                                                                     unsigned long long* __restrict__ sums) {
  __shared__ uint64_t s_pat[kPatternLdsCap / 8];
  Literals l;
  l.pat = stage_pattern(s_pat, g_pat, m);
  l.m = m;
  l.pfx = pattern_prefix(l.pat, m);
  l.rep = nullptr;
  l.r = r;
  const uint64_t d = reinterpret_cast<uint64_t>(data);
  const int lane = lane_id();
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  // a wave takes `chunk` consecutive rows a step, one after the other, and lane i keeps row i's length and count: they are
  // stored coalesced and the step's bytes reach their sum in one atomic.  chunk divides 64, so the rows of a step share a
  // validity word and a sum.
  for (int64_t base = wave * chunk; base < n; base += nwaves * chunk) {
    const uint64_t ok = load_word(valid, base >> 6) >> (base & 63);     // bit i: row base + i is valid (0 past the end)
    const int64_t row = base + lane;
    const bool mine = lane < chunk && ((ok >> lane) & 1);
    int64_t len = 0, c = 0;
    if (mine) len = static_cast<int64_t>(offsets[row + 1]) - static_cast<int64_t>(offsets[row]);
    for (int i = 0; cap != 0 && i < chunk; ++i) {
      if (!((ok >> i) & 1)) continue;                                   // (wave-uniform)
      const int64_t s_off = offsets[base + i], e_off = offsets[base + i + 1];
      if (e_off - s_off < m) continue;
      const int64_t found = wave_count_matches(d + static_cast<uint64_t>(s_off), d + static_cast<uint64_t>(e_off), l, cap);
      if (lane == i) c = found;
    }
    const int64_t out_len = len + c * (r - m);
    if (lane < chunk && row < n) {
      lens[row] = static_cast<O>(out_len);
      cnt[row] = static_cast<O>(c);
    }
    const uint64_t total = wave_reduce_sum_u64(static_cast<uint64_t>(out_len));
    if (lane == 0 && total != 0) atomicAdd(&sums[base / kBinRows], static_cast<unsigned long long>(total));
  }
}

template <typename O>
__global__ __launch_bounds__(kBlock) void replace_write_waves_kernel(Bits valid, const O* __restrict__ offsets, const uint8_t* __restrict__ data,
                                                                     int64_t n, const uint8_t* __restrict__ g_pat, int64_t m,
                                                                     const uint8_t* __restrict__ g_rep, int64_t r, const O* __restrict__ cnt,
                                                                     const O* __restrict__ out_offsets, uint8_t* __restrict__ out) {
  __shared__ uint64_t s_pat[kPatternLdsCap / 8];
  __shared__ uint64_t s_rep[kPatternLdsCap / 8];
  Literals l;
  l.pat = stage_pattern(s_pat, g_pat, m);
  l.m = m;
  l.pfx = pattern_prefix(l.pat, m);
  l.rep = stage_pattern(s_rep, g_rep, r);
  l.r = r;
  const uint64_t d = reinterpret_cast<uint64_t>(data);
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t row = wave; row < n; row += nwaves) {                // (wave-uniform from here on)
    if (!((load_word(valid, row >> 6) >> (row & 63)) & 1)) continue;
    const int64_t s_off = offsets[row], e_off = offsets[row + 1];
    if (e_off <= s_off) continue;
    wave_write_row(d + static_cast<uint64_t>(s_off), d + static_cast<uint64_t>(e_off), l, cnt[row], out + static_cast<int64_t>(out_offsets[row]));
  }
}

// the consecutive rows a wave of the count pass takes a step: the smallest power of two that lets the largest grid cover
// the rows in one step, 64 at most — few long rows still give every wave of the machine a row
int waves_chunk(int64_t n) {
  const int64_t want = ceil_div(n, static_cast<int64_t>(device_cus()) * 8 * kWavesPerBlock);
  int chunk = 1;
  while (chunk < want && chunk < kWave) chunk <<= 1;
  return chunk;
}

// step one (the `produce` of offsets_call; the workspace's second part holds the counts)
template <typename O>
int replace_offsets_launch(const Column& c, bool waves, const uint8_t* pat, int64_t m, int64_t r, int64_t cap, O* lens, O* cnt,
                           unsigned long long* sums, hipStream_t st) {
  const O* offsets = static_cast<const O*>(c.offsets);
  if (waves) {
    const int chunk = waves_chunk(c.n);
    hipLaunchKernelGGL(replace_count_waves_kernel<O>, dim3(waves_grid(c.n, chunk)), dim3(kBlock), 0, st, c.valid, offsets, c.data, c.n, pat, m,
                       r, cap, chunk, lens, cnt, sums);
    ARX_CHECK_LAUNCH("replace_count_waves_kernel");
    g_replace_wave_launches.fetch_add(1, std::memory_order_relaxed);
  } else {
    hipLaunchKernelGGL(replace_count_rows_kernel<O>, dim3(rows_grid(c.n)), dim3(kBlock), 0, st, c.valid, offsets, c.data, c.n, pat, m, r,
                       cap, lens, cnt, sums);
    ARX_CHECK_LAUNCH("replace_count_rows_kernel");
    g_replace_row_launches.fetch_add(1, std::memory_order_relaxed);
  }
  return ARX_OK;
}

template <typename O>
int replace_data_launch(const Column& c, bool waves, const uint8_t* pat, int64_t m, const uint8_t* rep, int64_t r, const void* ws,
                        const void* out_offsets, void* out_data, hipStream_t st) {
  const O* offsets = static_cast<const O*>(c.offsets);
  const O* cnt = reinterpret_cast<const O*>(static_cast<const uint8_t*>(ws) + bin_sums_bytes(c.n));
  if (waves) {
    hipLaunchKernelGGL(replace_write_waves_kernel<O>, dim3(waves_grid(c.n)), dim3(kBlock), 0, st, c.valid, offsets, c.data, c.n, pat, m, rep,
                       r, cnt, static_cast<const O*>(out_offsets), static_cast<uint8_t*>(out_data));
    ARX_CHECK_LAUNCH("replace_write_waves_kernel");
    g_replace_wave_launches.fetch_add(1, std::memory_order_relaxed);
  } else {
    hipLaunchKernelGGL(replace_write_rows_kernel<O>, dim3(rows_grid(c.n)), dim3(kBlock), 0, st, c.valid, offsets, c.data, c.n, pat, m, rep, r,
                       cnt, static_cast<const O*>(out_offsets), static_cast<uint8_t*>(out_data));
    ARX_CHECK_LAUNCH("replace_write_rows_kernel");
    g_replace_row_launches.fetch_add(1, std::memory_order_relaxed);
  }
  return ARX_OK;
}

// the checks the two calls share
int check_replace(const char* who, const ArxBinarySpan* values, int offset_width, const void* pattern, int64_t pattern_length,
                  bool replacement_missing, int64_t replacement_length, int path) {
  int rc = check_path(who, path);
  if (rc == ARX_OK) rc = check_common(who, values, offset_width);
  if (rc != ARX_OK) return rc;
  if (pattern_length <= 0) {
    set_error("%s: pattern_length %lld is not positive (the empty pattern has no device kernel)", who, static_cast<long long>(pattern_length));
    return ARX_INVALID;
  }
  if (replacement_length < 0) {
    set_error("%s: negative replacement_length %lld", who, static_cast<long long>(replacement_length));
    return ARX_INVALID;
  }
  if (pattern == nullptr || replacement_missing) {
    set_error("%s: NULL pattern or replacement", who);
    return ARX_INVALID;
  }
  return ARX_OK;
}

}  // namespace

static const CounterRow kStringReplaceCounters[] = {
    {"string_replace_row_launches", &g_replace_row_launches},
    {"string_replace_wave_launches", &g_replace_wave_launches},
};
CounterTable string_replace_counters() { return counter_table(kStringReplaceCounters); }

}  // namespace arx

using namespace arx;

extern "C" {

size_t arx_replace_substring_workspace_bytes(int64_t length, int offset_width) {
  return bin_workspace_bytes(length, offset_width == 8 ? 8 : 4);
}

int arx_replace_substring_offsets(const ArxBinarySpan* values, int offset_width, const void* pattern, int64_t pattern_length,
                                  int64_t replacement_length, int64_t max_replacements, int64_t data_bytes_hint, int path, void* ws,
                                  size_t ws_bytes, void* out_offsets, int64_t* out_total_bytes, void* stream) {
  int rc = check_offsets_arguments("replace_substring_offsets", values, out_offsets, out_total_bytes);
  if (rc == ARX_OK) rc = check_replace("replace_substring_offsets", values, offset_width, pattern, pattern_length, false, replacement_length, path);
  if (rc != ARX_OK) return rc;
  const int64_t cap = max_replacements < 0 ? kNoCap : max_replacements;
  const auto* pat = static_cast<const uint8_t*>(pattern);
  return offsets_call("replace_substring_offsets", "arx_replace_substring_workspace_bytes", values, offset_width, ws, ws_bytes, out_offsets,
                      out_total_bytes, "replacing substrings of a binary array", as_stream(stream),
                      [&](const Column& c, auto* lens, auto* cnt, unsigned long long* sums, hipStream_t st) {
                        const bool waves = take_waves(path, mean_bytes(data_bytes_hint, c.n));
                        return replace_offsets_launch(c, waves, pat, pattern_length, replacement_length, cap, lens, cnt, sums, st);
                      });
}

int arx_replace_substring_data(const ArxBinarySpan* values, int offset_width, const void* pattern, int64_t pattern_length,
                               const void* replacement, int64_t replacement_length, int64_t max_replacements, int path, const void* ws,
                               size_t ws_bytes, const void* out_offsets, int64_t total_bytes, void* out_data, void* stream) {
  if (values == nullptr) {
    set_error("replace_substring_data: NULL values");
    return ARX_INVALID;
  }
  int rc = check_replace("replace_substring_data", values, offset_width, pattern, pattern_length,
                         replacement == nullptr && replacement_length > 0, replacement_length, path);
  if (rc != ARX_OK) return rc;
  if (total_bytes < 0) {
    set_error("replace_substring_data: negative total_bytes %lld", static_cast<long long>(total_bytes));
    return ARX_INVALID;
  }
  const int64_t n = values->length;
  if (n == 0 || total_bytes == 0) return ARX_OK;
  if (out_offsets == nullptr || out_data == nullptr || values->data == nullptr || values->offsets == nullptr) {
    set_error("replace_substring_data: NULL out_offsets, out_data, or offsets or data of values");
    return ARX_INVALID;
  }
  rc = check_offsets_workspace("replace_substring_data", "arx_replace_substring_workspace_bytes", ws, ws_bytes, n, offset_width);
  if (rc != ARX_OK) return rc;
  (void)max_replacements;   // (the workspace holds every row's accepted count, the cap applied)
  const Column c = column_of(values, offset_width);
  const bool waves = take_waves(path, total_bytes / n);
  hipStream_t st = as_stream(stream);
  const auto* pat = static_cast<const uint8_t*>(pattern);
  const auto* rep = static_cast<const uint8_t*>(replacement);
  return with_offset_type(offset_width, [&](auto o) {
    return replace_data_launch<decltype(o)>(c, waves, pat, pattern_length, rep, replacement_length, ws, out_offsets, out_data, st);
  });
}

}  // extern "C"

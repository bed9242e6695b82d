// Trimming of utf8 / large_utf8 columns: the twelve {ascii,utf8}_{,l,r}trim{,_whitespace} functions
// (compute/kernels/scalar_string_ascii.cc / scalar_string_utf8.cc).  A trimmed row is a sub-range of its row, so this is
// step one of a slice with another first kernel: it writes every row's source begin and length and the sums of
// binary_scan_copy.h, bin_scan_lengths makes the offsets, and arx_string_slice_data (string_slice.hip) is the copy.
//
// Sets.  ASCII_WHITESPACE: the bytes 9 .. 13 and 32.  BYTES: any set of bytes, four 64-bit words.  Both trim bytes.
// UTF8_WHITESPACE: the 29 codepoints the reference's IsSpaceCharacterUnicode accepts (9 .. 13, 0x1C .. 0x20 and
// utf8_whitespace_above_ascii below).  CODEPOINTS: up to ARX_TRIM_MAX_CODEPOINTS distinct codepoints, kernel arguments.
// Both trim UNITS, defined on any bytes so that a result never leaves its row (the lead / continuation rule of
// string_slice.hip, extended by a value):
//   front unit  a continuation byte (0b10xxxxxx) alone, without a value; else a lead and the continuation bytes after
//               it inside the row, at most three;
//   back unit   step back over at most three continuation bytes; if the byte reached is one too (or the row's start was
//               reached on one) the row's last byte alone, without a value; else from that lead to the row's end;
//   value       only when the unit's length is the one its lead declares (0xxxxxxx 1, 110xxxxx 2, 1110xxxx 3,
//               11110xxx 4, any other lead none) and the decoded value is not below 0 / 0x80 / 0x800 / 0x10000.
// Trimming advances over a unit that has a value in the set and stops at any other.  Left first, then right on what is
// left.  Valid UTF-8 gives the reference's result; where the reference raises "Invalid UTF8 sequence in input" the
// trim stops and the row is returned from there.
//
// One lane per row.  Every set is first a per-byte question with a bit-7 answer for the 16 bytes of an aligned granule
// (granule rule as string_slice.hip: only granules that hold a byte of a valid row are loaded): ASCII whitespace by
// 64-bit word arithmetic, a byte set by 16 look-ups in its words, and for the two UTF-8 sets their members below 0x80
// the same way.  __ffsll / clz of the complement find the first / last byte that stops the walk, so a row with nothing
// to trim costs one granule a side and a run of trimmable bytes one step a granule.  The UTF-8 sets decode a unit only
// where the walk stopped on a byte >= 0x80; its bytes are the row's own, read one by one.
#include "string_rows.h"

namespace arx {

namespace {

std::atomic<int64_t> g_trim_launches{0};

// the members >= 0x80 of the reference's whitespace set (those below: 9 .. 13 and 0x1C .. 0x20)
__device__ __forceinline__ bool utf8_whitespace_above_ascii(uint32_t v) {
  return v == 0x85 || v == 0xA0 || v == 0x1680 || (v >= 0x2000 && v <= 0x200A) || v == 0x2028 || v == 0x2029 || v == 0x202F ||
         v == 0x205F || v == 0x3000;
}

// the set of a call, by value: `bytes` answers for single bytes (BYTES: all 256; CODEPOINTS: the members below 0x80),
// wide[0, nwide) are the CODEPOINTS members from 0x80 on
struct TrimSet {
  uint64_t bytes[4];
  uint32_t nwide;
  uint32_t wide[ARX_TRIM_MAX_CODEPOINTS];
};

// bit 7 of every byte x of w with lo <= (x & 0x7F) <= hi (0 <= lo <= hi <= 0x7F); no carry crosses a byte
__device__ __forceinline__ uint64_t low7_in_range(uint64_t w7, uint32_t lo, uint32_t hi) {
  constexpr uint64_t kOnes = 0x0101010101010101ull;
  const uint64_t ge_lo = w7 + kOnes * (0x80 - lo);        // bit 7: x >= lo
  const uint64_t gt_hi = w7 + kOnes * (0x7F - hi);        // bit 7: x > hi
  return ge_lo & ~gt_hi & kBit7;
}

// bit 7 of every byte of w that, taken alone, is in the set
template <int KIND>
__device__ __forceinline__ uint64_t bytes_in_set(uint64_t w, const TrimSet& set) {
  if constexpr (KIND == ARX_TRIM_ASCII_WHITESPACE || KIND == ARX_TRIM_UTF8_WHITESPACE) {
    const uint64_t w7 = w & ~kBit7;
    uint64_t in = low7_in_range(w7, 9, 13);
    if constexpr (KIND == ARX_TRIM_ASCII_WHITESPACE) in |= low7_in_range(w7, 32, 32);
    else in |= low7_in_range(w7, 0x1C, 0x20);
    return in & ~w;                                        // (a byte >= 0x80 is in neither)
  } else {
    uint64_t in = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t x = static_cast<uint32_t>(w >> (8 * j)) & 0xFF;
      uint64_t word;
      if constexpr (KIND == ARX_TRIM_BYTES) word = (x & 0x80) ? ((x & 0x40) ? set.bytes[3] : set.bytes[2]) : ((x & 0x40) ? set.bytes[1] : set.bytes[0]);
      else word = (x & 0x80) ? 0 : ((x & 0x40) ? set.bytes[1] : set.bytes[0]);
      in |= ((word >> (x & 63)) & 1) << (8 * j + 7);
    }
    return in;
  }
}

template <int KIND>
__device__ __forceinline__ bool codepoint_in_set(uint32_t v, const TrimSet& set) {
  if constexpr (KIND == ARX_TRIM_UTF8_WHITESPACE) {
    return utf8_whitespace_above_ascii(v);
  } else {
    bool in = false;
    for (uint32_t i = 0; i < set.nwide; ++i) in = in || set.wide[i] == v;   // (uniform loop, the members sit in SGPRs)
    return in;
  }
}

__device__ __forceinline__ bool is_continuation(uint32_t x) { return (x & 0xC0) == 0x80; }

// the value of the unit [u, u + len) of 1 .. 4 bytes whose first byte is a lead >= 0x80, or no value (false)
__device__ __forceinline__ bool unit_value(const uint8_t* u, int len, uint32_t* value) {
  const uint32_t lead = u[0];
  const int declared = (lead >> 5) == 6 ? 2 : (lead >> 4) == 14 ? 3 : (lead >> 3) == 30 ? 4 : 0;
  if (declared == 0 || declared != len) return false;
  uint32_t v = lead & (0xFFu >> (declared + 1));
  for (int j = 1; j < declared; ++j) v = (v << 6) | (u[j] & 0x3F);
  *value = v;
  return v >= (declared == 2 ? 0x80u : declared == 3 ? 0x800u : 0x10000u);
}

// the 16 bytes of the aligned granule at address g as the bit-7 mask of its bytes inside [s, e) that are NOT in the set
template <int KIND>
__device__ __forceinline__ void granule_stops(uint64_t g, uint64_t s, uint64_t e, const TrimSet& set, uint64_t* lo, uint64_t* hi) {
  const uint4 q = *reinterpret_cast<const uint4*>(g);
  const uint64_t wlo = q.x | (static_cast<uint64_t>(q.y) << 32), whi = q.z | (static_cast<uint64_t>(q.w) << 32);
  const int64_t from = g < s ? static_cast<int64_t>(s - g) : 0, to = g + 16 > e ? static_cast<int64_t>(e - g) : 16;
  *lo = ~bytes_in_set<KIND>(wlo, set) & byte_range_bit7(from, to);
  *hi = ~bytes_in_set<KIND>(whi, set) & byte_range_bit7(from - 8, to - 8);
}

constexpr bool kind_is_utf8(int kind) { return kind == ARX_TRIM_UTF8_WHITESPACE || kind == ARX_TRIM_CODEPOINTS; }

// the address where the left trim of the row [s, e) (addresses, s < e) ends
template <int KIND>
__device__ __forceinline__ uint64_t trim_front(uint64_t s, uint64_t e, const TrimSet& set) {
  uint64_t p = s;
  while (p < e) {
    const uint64_t g = p & ~uint64_t(15);
    uint64_t lo, hi;
    granule_stops<KIND>(g, p, e, set, &lo, &hi);
    if ((lo | hi) == 0) {                                  // every byte of the row in this granule is in the set
      p = g + 16 < e ? g + 16 : e;
      continue;
    }
    p = g + (lo != 0 ? (__ffsll(static_cast<unsigned long long>(lo)) - 1) >> 3 : 8 + ((__ffsll(static_cast<unsigned long long>(hi)) - 1) >> 3));
    if constexpr (!kind_is_utf8(KIND)) {
      break;
    } else {
      const uint8_t* u = reinterpret_cast<const uint8_t*>(p);
      if (u[0] < 0x80) break;                              // a single byte outside the set
      if (is_continuation(u[0])) {
        // a unit without a value; and if the byte passed just before it is below 0x80, that byte's unit reaches up to
        // here and has none either (the per-byte answer could not know)
        if (p > s && u[-1] < 0x80) --p;
        break;
      }
      int len = 1;
      while (len < 4 && p + len < e && is_continuation(u[len])) ++len;
      uint32_t v;
      if (!unit_value(u, len, &v) || !codepoint_in_set<KIND>(v, set)) break;
      p += len;
    }
  }
  return p;
}

// the address where the right trim of the row [p, e) (addresses, p < e) begins
template <int KIND>
__device__ __forceinline__ uint64_t trim_back(uint64_t p, uint64_t e, const TrimSet& set) {
  while (e > p) {
    const uint64_t g = (e - 1) & ~uint64_t(15);
    uint64_t lo, hi;
    granule_stops<KIND>(g, p, e, set, &lo, &hi);
    if ((lo | hi) == 0) {
      e = g > p ? g : p;
      continue;
    }
    // the last byte that stops the walk: (63 - clz) / 8 is the byte of the highest set bit
    const uint64_t last = g + (hi != 0 ? 8 + ((63 - __builtin_clzll(hi)) >> 3) : (63 - __builtin_clzll(lo)) >> 3);
    e = last + 1;
    if constexpr (!kind_is_utf8(KIND)) {
      break;
    } else {
      if (*reinterpret_cast<const uint8_t*>(last) < 0x80) break;
      uint64_t lead = last;
      for (int k = 0; k < 3 && lead > p && is_continuation(*reinterpret_cast<const uint8_t*>(lead)); ++k) --lead;
      const uint8_t* u = reinterpret_cast<const uint8_t*>(lead);
      if (is_continuation(u[0])) break;
      uint32_t v;
      if (u[0] < 0x80 || !unit_value(u, static_cast<int>(e - lead), &v) || !codepoint_in_set<KIND>(v, set)) break;
      e = lead;
    }
  }
  return e;
}

// step one of a trim, one lane per row (the contract of binary_scan_copy.h): lens[row] = the trimmed row's length,
// src[row] = the index of its first byte in data, sums[row / kBinRows] += the length, one atomic a wave
template <typename O, int SIDES, int KIND>
__global__ __launch_bounds__(kBlock) void trim_rows_kernel(Bits valid, const O* __restrict__ offsets, const uint8_t* __restrict__ data,
                                                           int64_t n, const TrimSet set, O* __restrict__ lens, O* __restrict__ src,
                                                           unsigned long long* __restrict__ sums) {
  const int lane = lane_id();
  const uint64_t d = reinterpret_cast<uint64_t>(data);
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kBlock; base < n; base += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t row = base + threadIdx.x;
    const bool ok = (load_word(valid, row >> 6) >> lane) & 1;       // 0 past the end
    int64_t begin = 0, end = 0;
    if (row < n) {
      begin = end = offsets[row];
      if (ok) {
        end = offsets[row + 1];
        if (end > begin) {                                          // (else no referenced byte, and data may be NULL)
          uint64_t p = d + static_cast<uint64_t>(begin), e = d + static_cast<uint64_t>(end);
          if constexpr ((SIDES & ARX_TRIM_LEFT) != 0) p = trim_front<KIND>(p, e, set);
          if constexpr ((SIDES & ARX_TRIM_RIGHT) != 0) e = trim_back<KIND>(p, e, set);
          begin = static_cast<int64_t>(p - d);
          end = static_cast<int64_t>(e - d);
        }
      }
      lens[row] = static_cast<O>(end - begin);
      src[row] = static_cast<O>(begin);
    }
    const uint64_t total = wave_reduce_sum_u64(static_cast<uint64_t>(end - begin));
    if (lane == 0 && total != 0) atomicAdd(&sums[(row - lane) / kBinRows], static_cast<unsigned long long>(total));
  }
}

// step one of a trim (the `produce` of offsets_call), by its sides and its set kind
template <typename O, int SIDES, int KIND>
int trim_launch(const Column& c, const TrimSet& set, O* lens, O* src, unsigned long long* sums, hipStream_t st) {
  hipLaunchKernelGGL((trim_rows_kernel<O, SIDES, KIND>), dim3(rows_grid(c.n)), dim3(kBlock), 0, st, c.valid, static_cast<const O*>(c.offsets),
                     c.data, c.n, set, lens, src, sums);
  ARX_CHECK_LAUNCH("trim_rows_kernel");
  g_trim_launches.fetch_add(1, std::memory_order_relaxed);
  return ARX_OK;
}

template <typename O, int SIDES>
int trim_by_kind(int kind, const Column& c, const TrimSet& set, O* lens, O* src, unsigned long long* sums, hipStream_t st) {
  switch (kind) {
    case ARX_TRIM_ASCII_WHITESPACE: return trim_launch<O, SIDES, ARX_TRIM_ASCII_WHITESPACE>(c, set, lens, src, sums, st);
    case ARX_TRIM_UTF8_WHITESPACE: return trim_launch<O, SIDES, ARX_TRIM_UTF8_WHITESPACE>(c, set, lens, src, sums, st);
    case ARX_TRIM_BYTES: return trim_launch<O, SIDES, ARX_TRIM_BYTES>(c, set, lens, src, sums, st);
    default: return trim_launch<O, SIDES, ARX_TRIM_CODEPOINTS>(c, set, lens, src, sums, st);
  }
}

template <typename O>
int trim_by_sides(int sides, int kind, const Column& c, const TrimSet& set, O* lens, O* src, unsigned long long* sums, hipStream_t st) {
  switch (sides) {
    case ARX_TRIM_LEFT: return trim_by_kind<O, ARX_TRIM_LEFT>(kind, c, set, lens, src, sums, st);
    case ARX_TRIM_RIGHT: return trim_by_kind<O, ARX_TRIM_RIGHT>(kind, c, set, lens, src, sums, st);
    default: return trim_by_kind<O, ARX_TRIM_BOTH>(kind, c, set, lens, src, sums, st);
  }
}

// the host `set` of a call as a TrimSet; more than ARX_TRIM_MAX_CODEPOINTS distinct codepoints: ARX_NOT_IMPLEMENTED
int make_set(int kind, const void* set, int64_t set_length, TrimSet* out) {
  *out = TrimSet{};
  if (kind == ARX_TRIM_BYTES) {
    const auto* b = static_cast<const uint8_t*>(set);
    for (int64_t i = 0; i < set_length; ++i) out->bytes[b[i] >> 6] |= uint64_t(1) << (b[i] & 63);
  } else if (kind == ARX_TRIM_CODEPOINTS) {
    const auto* cp = static_cast<const uint32_t*>(set);
    int64_t distinct = 0;
    for (int64_t i = 0; i < set_length; ++i) {
      const uint32_t v = cp[i];
      if (v < 0x80) {
        const uint64_t bit = uint64_t(1) << (v & 63);
        if ((out->bytes[v >> 6] & bit) == 0) ++distinct;
        out->bytes[v >> 6] |= bit;
      } else if (std::find(out->wide, out->wide + out->nwide, v) == out->wide + out->nwide) {
        ++distinct;
        if (out->nwide < ARX_TRIM_MAX_CODEPOINTS) out->wide[out->nwide++] = v;
      }
      if (distinct > ARX_TRIM_MAX_CODEPOINTS) {
        set_error("string_trim_offsets: more than %d distinct codepoints to trim have no device kernel", ARX_TRIM_MAX_CODEPOINTS);
        return ARX_NOT_IMPLEMENTED;
      }
    }
  }
  return ARX_OK;
}

}  // namespace

static const CounterRow kStringTrimCounters[] = {
    {"string_trim_launches", &g_trim_launches},
};
CounterTable string_trim_counters() { return counter_table(kStringTrimCounters); }

}  // namespace arx

using namespace arx;

extern "C" {

int arx_string_trim_offsets(const ArxBinarySpan* values, int offset_width, int sides, int set_kind, const void* set, int64_t set_length,
                            void* ws, size_t ws_bytes, void* out_offsets, int64_t* out_total_bytes, void* stream) {
  int rc = check_offsets_arguments("string_trim_offsets", values, out_offsets, out_total_bytes);
  if (rc != ARX_OK) return rc;
  if (sides != ARX_TRIM_LEFT && sides != ARX_TRIM_RIGHT && sides != ARX_TRIM_BOTH) {
    set_error("string_trim_offsets: sides %d is not 1 (left), 2 (right) or 3 (both)", sides);
    return ARX_INVALID;
  }
  if (set_kind < ARX_TRIM_ASCII_WHITESPACE || set_kind > ARX_TRIM_CODEPOINTS) {
    set_error("string_trim_offsets: set_kind %d is not 0 (ascii whitespace), 1 (utf8 whitespace), 2 (bytes) or 3 (codepoints)", set_kind);
    return ARX_INVALID;
  }
  rc = check_common("string_trim_offsets", values, offset_width);
  if (rc != ARX_OK) return rc;
  const bool takes_set = set_kind == ARX_TRIM_BYTES || set_kind == ARX_TRIM_CODEPOINTS;
  if (takes_set && (set_length < 0 || (set == nullptr && set_length > 0))) {
    set_error("string_trim_offsets: negative set_length %lld, or a NULL set of that length", static_cast<long long>(set_length));
    return ARX_INVALID;
  }
  TrimSet trim_set;
  rc = make_set(set_kind, set, set_length, &trim_set);
  if (rc != ARX_OK) return rc;
  return offsets_call("string_trim_offsets", "arx_string_slice_workspace_bytes", values, offset_width, ws, ws_bytes, out_offsets,
                      out_total_bytes, "trimming a string array", as_stream(stream),
                      [&](const Column& c, auto* lens, auto* src, unsigned long long* sums, hipStream_t st) {
                        return trim_by_sides(sides, set_kind, c, trim_set, lens, src, sums, st);
                      });
}

}  // extern "C"

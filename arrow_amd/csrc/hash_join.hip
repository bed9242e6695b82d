// Hash join: the kernels of an equi-join that come after the Grouper (acero/hash_join_node.cc, SwissJoin in
// acero/swiss_join.cc).  Key rows -> dense ids stays with the Grouper (grouper.hip): the build (right) side is consumed,
// giving every build row a uint32 id; the probe (left) side is looked up, giving an id or null.  Under JoinKeyCmp::EQ a
// row with a null in any key column matches nothing: the caller folds the key columns' validity into the id validity
// (arx_hash_join_key_validity).  What is left is integer work on the ids:
//
//   build index   group_offsets[G + 1] = exclusive scan of a histogram of the valid build ids (this file); the rows of
//                 each group in ascending row order come from the stable sort of the ids (arx_sort_indices on uint32,
//                 nulls at the end), so no stable placement kernel is needed: the sort IS the placement.
//   probe count   one lane per probe row: its output rows from its group's size and the join type; the groups it hits
//                 are marked in a byte-per-group array with a plain store of 1 (idempotent, no atomics).  An exclusive
//                 scan gives per-row output offsets and the total, the one host read-back that sizes the output.
//   expand        load-balanced over OUTPUT slots: a workgroup owns 512 consecutive slots, finds the probe rows of its
//                 first and last slot by binary search in the scanned offsets, and every lane finds its two slots' rows
//                 inside that (short) range.  One hot key with 10^6 build rows is spread over 2000 workgroups like any
//                 other run of slots.  Each lane writes its two (left, right) pairs as 16-byte stores; the right side's
//                 validity is two ballots per wave, interleaved into two 64-bit words.
//   build side    the matched bytes become a mask over build rows (matched / unmatched, null keys counted unmatched);
//                 the caller compacts it with arx_mask_to_indices and appends the rows with a null left index.
//   residual      HashJoinNodeOptions::filter: a key-equal pair is a match only where the filter is true (null: no match).
//   filter        The caller expands the CANDIDATES as an inner join, evaluates the filter over the T candidate slots and
//                 hands in the boolean column.  filter count: pass word = value AND validity, one popcount per 64-slot
//                 word, scanned (the three launches above) into P: passing slots before slot j in O(1).  A probe row's
//                 passing pairs are P(offsets[i + 1]) - P(offsets[i]); its output rows follow by join type and are
//                 scanned into the new offsets (the one more read-back).  Passing slots mark build ROWS (a byte each,
//                 plain store of 1): the filter tells apart rows that share a key.  filter compact: one lane per
//                 candidate slot, slot j of row r lands at new_offsets[r] + P(j) - P(offsets[r]); one lane per probe row
//                 writes the (row, null) slot of a left / full outer row without a passing pair.  All work is per slot
//                 or per row, O(1) each: a hot key costs per slot what any other input costs.  Byte flags become the
//                 masks of semi / anti joins and of the right-only tail (flags_to_mask, either polarity).
#include "arx_common.h"

#include <cstring>

namespace arx {

namespace {

enum JoinType {   // arrow::acero::JoinType, in the enum's order
  kLeftSemi = 0, kRightSemi = 1, kLeftAnti = 2, kRightAnti = 3, kInner = 4, kLeftOuter = 5, kRightOuter = 6, kFullOuter = 7
};

constexpr int kScanItems = 16;                            // elements per lane of one scan block
constexpr int64_t kScanBlock = int64_t(kBlock) * kScanItems;
constexpr size_t kScanHeader = 64;                         // ws: total (u64), overflow flag (u64), then the block sums
constexpr int kExpandSlots = 2 * kBlock;                  // output slots per expand workgroup: two per lane
constexpr unsigned kMaxGrid = 1u << 20;

// two int64 as one 16-byte store (the carrier is the 4 x u32 vector of arx_common.h)
__device__ __forceinline__ void store_pair(int64_t* p, int64_t a, int64_t b) {
  arx_u32x4 v;
  v[0] = uint32_t(uint64_t(a)); v[1] = uint32_t(uint64_t(a) >> 32);
  v[2] = uint32_t(uint64_t(b)); v[3] = uint32_t(uint64_t(b) >> 32);
  *reinterpret_cast<arx_u32x4*>(p) = v;
}

__device__ __forceinline__ bool valid_bit(const uint64_t* bits, int64_t i) {
  return bits == nullptr || ((bits[i >> 6] >> (i & 63)) & 1);
}

__device__ __forceinline__ bool marks_build(int jt) {
  return jt == kRightSemi || jt == kRightAnti || jt == kRightOuter || jt == kFullOuter;
}

// ----------------------------------------------------------------------------------------------- exclusive scan
// In place: a[0..n) -> exclusive prefix sums, a[n] = total.  Three launches (block sums, one workgroup over the block
// sums, block scans), so no workgroup waits on another.  A total above INT64_MAX sets the overflow flag instead.
__device__ __forceinline__ uint64_t block_exclusive_scan(uint64_t v, uint64_t* lds_waves, uint64_t* block_total) {
  const int lane = lane_id(), wave = threadIdx.x / kWave;
  const uint64_t incl = wave_inclusive_scan_u64(v);
  if (lane == kWave - 1) lds_waves[wave] = incl;
  __syncthreads();
  uint64_t before = 0, all = 0;
  for (int w = 0; w < kWavesPerBlock; ++w) {
    const uint64_t s = lds_waves[w];
    if (w < wave) before += s;
    all += s;
  }
  __syncthreads();
  *block_total = all;
  return before + incl - v;
}

__global__ void __launch_bounds__(kBlock) scan_block_sums_kernel(const int64_t* a, int64_t n, uint64_t* sums) {
  __shared__ uint64_t lds[kWavesPerBlock];
  const int64_t base = int64_t(blockIdx.x) * kScanBlock;
  uint64_t s = 0;
#pragma unroll
  for (int i = 0; i < kScanItems; ++i) {
    const int64_t j = base + int64_t(i) * kBlock + threadIdx.x;
    if (j < n) s += static_cast<uint64_t>(a[j]);
  }
  s = wave_reduce_sum_u64(s);
  if (lane_id() == 0) lds[threadIdx.x / kWave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t t = 0;
    for (int w = 0; w < kWavesPerBlock; ++w) t += lds[w];
    sums[blockIdx.x] = t;
  }
}

// One workgroup: sums[b] -> exclusive prefix; header = {total, overflow}; a[n] = total.
__global__ void __launch_bounds__(kBlock) scan_block_offsets_kernel(uint64_t* header, uint64_t* sums, int64_t num_blocks,
                                                                    int64_t* a, int64_t n) {
  __shared__ uint64_t lds[kWavesPerBlock];
  uint64_t carry = 0;
  bool overflow = false;
  for (int64_t c = 0; c < num_blocks; c += kBlock) {
    const int64_t b = c + threadIdx.x;
    const uint64_t v = b < num_blocks ? sums[b] : 0;
    uint64_t chunk = 0;
    const uint64_t ex = block_exclusive_scan(v, lds, &chunk);
    if (b < num_blocks) sums[b] = carry + ex;
    if (chunk > uint64_t(INT64_MAX) - carry) overflow = true;   // block sums are < 2^52: the chunk itself cannot wrap
    carry = overflow ? uint64_t(INT64_MAX) : carry + chunk;
  }
  if (threadIdx.x == 0) {
    header[0] = carry;
    header[1] = overflow ? 1 : 0;
    a[n] = static_cast<int64_t>(carry);
  }
}

__global__ void __launch_bounds__(kBlock) scan_apply_kernel(int64_t* a, int64_t n, const uint64_t* sums) {
  __shared__ uint64_t lds[kWavesPerBlock];
  const int64_t first = int64_t(blockIdx.x) * kScanBlock + int64_t(threadIdx.x) * kScanItems;
  uint64_t v[kScanItems];
  uint64_t mine = 0;
#pragma unroll
  for (int i = 0; i < kScanItems; ++i) {
    v[i] = first + i < n ? static_cast<uint64_t>(a[first + i]) : 0;
    mine += v[i];
  }
  uint64_t unused = 0;
  uint64_t run = sums[blockIdx.x] + block_exclusive_scan(mine, lds, &unused);
#pragma unroll
  for (int i = 0; i < kScanItems; ++i) {
    if (first + i < n) a[first + i] = static_cast<int64_t>(run);
    run += v[i];
  }
}

size_t scan_ws_bytes(int64_t n) { return kScanHeader + 8 * size_t(ceil_div(n > 0 ? n : 1, kScanBlock)); }

int scan_in_place(int64_t* a, int64_t n, void* ws, size_t ws_bytes, hipStream_t st) {
  if (ws == nullptr || ws_bytes < scan_ws_bytes(n)) {
    set_error("hash join: workspace of %zu bytes, %zu needed", ws_bytes, scan_ws_bytes(n));
    return ARX_INVALID;
  }
  const int64_t blocks = ceil_div(n > 0 ? n : 1, kScanBlock);
  uint64_t* header = static_cast<uint64_t*>(ws);
  uint64_t* sums = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(ws) + kScanHeader);
  if (n > 0) {
    hipLaunchKernelGGL(scan_block_sums_kernel, dim3(unsigned(blocks)), dim3(kBlock), 0, st, a, n, sums);
    ARX_CHECK_LAUNCH("scan_block_sums_kernel");
  }
  hipLaunchKernelGGL(scan_block_offsets_kernel, dim3(1), dim3(kBlock), 0, st, header, sums, n > 0 ? blocks : 0, a, n);
  ARX_CHECK_LAUNCH("scan_block_offsets_kernel");
  if (n > 0) {
    hipLaunchKernelGGL(scan_apply_kernel, dim3(unsigned(blocks)), dim3(kBlock), 0, st, a, n, sums);
    ARX_CHECK_LAUNCH("scan_apply_kernel");
  }
  return ARX_OK;
}

unsigned grid_for(int64_t n) {
  const int64_t g = ceil_div(n > 0 ? n : 1, kBlock);
  return unsigned(g < int64_t(kMaxGrid) ? g : int64_t(kMaxGrid));
}

// ----------------------------------------------------------------------------------------------- key preparation
// out word w = (first ? ~0 : out[w]) & validity word w of the column (one lane per word)
__global__ void key_validity_kernel(Bits b, int64_t words, int first, uint64_t* out) {
  for (int64_t w = int64_t(blockIdx.x) * kBlock + threadIdx.x; w < words; w += int64_t(gridDim.x) * kBlock) {
    const uint64_t v = load_word(b, w);
    out[w] = first ? v : (out[w] & v);
  }
}

__global__ void bool_key_kernel(Bits bits, int64_t n, uint8_t* out) {
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kBlock) {
    out[i] = uint8_t((load_word(bits, i >> 6) >> (i & 63)) & 1);
  }
}

// ----------------------------------------------------------------------------------------------- build index
__global__ void group_histogram_kernel(const uint32_t* ids, const uint64_t* valid, int64_t n, int64_t num_groups,
                                       unsigned long long* counts) {
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kBlock) {
    const uint32_t g = ids[i];
    if (valid_bit(valid, i) && g < num_groups) atomicAdd(&counts[g], 1ull);
  }
}

// ----------------------------------------------------------------------------------------------- probe count
__global__ void probe_count_kernel(const uint32_t* ids, const uint64_t* valid, int64_t n, const int64_t* group_offsets,
                                   int64_t num_groups, int jt, uint8_t* matched, int64_t* counts) {
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kBlock) {
    const uint32_t g = ids[i];
    int64_t size = 0;
    if (valid_bit(valid, i) && g < num_groups) size = group_offsets[g + 1] - group_offsets[g];
    if (size > 0 && matched != nullptr && marks_build(jt)) matched[g] = 1;
    int64_t c;
    switch (jt) {
      case kLeftSemi: c = size > 0; break;
      case kLeftAnti: c = size == 0; break;
      case kInner:
      case kRightOuter: c = size; break;
      case kLeftOuter:
      case kFullOuter: c = size > 0 ? size : 1; break;
      default: c = 0; break;   // right semi / right anti: the probe only marks groups
    }
    counts[i] = c;
  }
}

// ----------------------------------------------------------------------------------------------- expand
// The probe row of slot j: the largest r in [lo, hi] with offsets[r] <= j.
__device__ __forceinline__ int64_t row_of_slot(const int64_t* offsets, int64_t lo, int64_t hi, int64_t j) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (offsets[mid] <= j) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ void __launch_bounds__(kBlock) expand_kernel(const int64_t* offsets, const uint32_t* ids, const uint64_t* valid,
                                                        int64_t n, const int64_t* group_offsets, const uint64_t* rows_by_group,
                                                        int jt, int64_t total, int64_t* out_left, int64_t* out_right,
                                                        uint64_t* out_right_valid) {
  __shared__ int64_t span[2];
  const bool with_right = out_right != nullptr;
  const int64_t tiles = (total + kExpandSlots - 1) / kExpandSlots;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {   // grid-stride over tiles: any total fits one launch
    const int64_t tile = t * kExpandSlots;
    __syncthreads();   // every lane has read the previous tile's span
    if (threadIdx.x < 2) {
      const int64_t last = tile + kExpandSlots - 1 < total ? tile + kExpandSlots - 1 : total - 1;
      span[threadIdx.x] = row_of_slot(offsets, 0, n - 1, threadIdx.x == 0 ? tile : last);
    }
    __syncthreads();
    const int64_t r_lo = span[0], r_hi = span[1];
    const int64_t j0 = tile + 2 * int64_t(threadIdx.x);
    int64_t lft[2] = {0, 0}, rgt[2] = {0, 0};
    bool rvalid[2] = {false, false};
    if (j0 < total) {
      int64_t r = r_lo;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int64_t j = j0 + s;
        if (j >= total) break;
        // each slot searches its own row: zero-count rows between the two slots cost no walk (log2 of the range)
        r = row_of_slot(offsets, r, r_hi, j);
        lft[s] = r;
        if (with_right) {
          const uint32_t g = ids[r];
          if (valid_bit(valid, r)) {
            const int64_t base = group_offsets[g], size = group_offsets[g + 1] - base;
            if (size > 0) {
              rgt[s] = static_cast<int64_t>(rows_by_group[base + (j - offsets[r])]);
              rvalid[s] = true;
            }
          }
        }
      }
      if (j0 + 1 < total) {
        store_pair(out_left + j0, lft[0], lft[1]);
        if (with_right) store_pair(out_right + j0, rgt[0], rgt[1]);
      } else {
        out_left[j0] = lft[0];
        if (with_right) out_right[j0] = rgt[0];
      }
    }
    if (out_right_valid != nullptr) {
      // lane l holds slots 2l, 2l + 1 of the wave's 128: even / odd ballots, interleaved into two words
      const uint64_t ev = __ballot(rvalid[0]), od = __ballot(rvalid[1]);
      const int64_t word = (tile + int64_t(threadIdx.x / kWave) * 2 * kWave) >> 6;
      const int64_t words = (total + 63) >> 6;
      const int lane = lane_id();
      if (lane < 2 && word + lane < words) {
        const uint64_t e = lane == 0 ? ev : ev >> 32, o = lane == 0 ? od : od >> 32;
        out_right_valid[word + lane] = spread32(e) | (spread32(o) << 1);
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------- build side
// bit i = ((row i's key is valid) && matched[id_i]) == want_matched; one ballot word per wave.
__global__ void __launch_bounds__(kBlock) build_mask_kernel(const uint32_t* ids, const uint64_t* valid, int64_t n,
                                                            const uint8_t* matched, int want_matched, uint64_t* out) {
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t base = int64_t(blockIdx.x) * kBlock; base < n; base += stride) {
    const int64_t i = base + threadIdx.x;
    bool hit = false;
    if (i < n) hit = (valid_bit(valid, i) && matched[ids[i]] != 0) == (want_matched != 0);
    const uint64_t word = __ballot(hit);
    if (lane_id() == 0 && (i >> 6) < ((n + 63) >> 6)) out[i >> 6] = word;
  }
}

// Slots [start, start + count): left index null, right index = rows[k].  Lane k also owns validity word k: the left
// validity is all ones below `start` and zero from it; the right validity keeps the expand's bits below `start` and is
// set from it.
__global__ void append_build_rows_kernel(const uint64_t* rows, int64_t count, int64_t start, int64_t* out_left,
                                         uint64_t* out_left_valid, int64_t* out_right, uint64_t* out_right_valid) {
  const int64_t end = start + count;
  const int64_t words = (end + 63) >> 6;
  const int64_t first_word = start >> 6;
  const int64_t lanes = count > words ? count : words;
  for (int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x; k < lanes; k += int64_t(gridDim.x) * kBlock) {
    if (k < count) {
      out_left[start + k] = 0;
      out_right[start + k] = static_cast<int64_t>(rows[k]);
    }
    if (k < words) {
      const int64_t lo = k << 6;
      const uint64_t below = lo + 64 <= start ? ~uint64_t(0) : (lo >= start ? 0 : low_mask64(int(start - lo)));
      if (out_left_valid != nullptr) out_left_valid[k] = below;
      if (out_right_valid != nullptr && k >= first_word) {
        const uint64_t upto = lo + 64 <= end ? ~uint64_t(0) : low_mask64(int(end - lo));
        out_right_valid[k] = (out_right_valid[k] & below) | (upto & ~below);
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------- residual filter
// P(x): the passing slots in [0, x), x in [0, T].  prefix has one entry per 64-slot word plus the total at [words].
__device__ __forceinline__ int64_t passing_before(const uint64_t* pass_bits, const int64_t* prefix, int64_t x) {
  const int64_t w = x >> 6;
  const int r = int(x & 63);
  int64_t p = prefix[w];
  if (r != 0) p += __popcll(pass_bits[w] & low_mask64(r));   // (r == 0: word w may be one past the last)
  return p;
}

__device__ __forceinline__ int64_t filtered_row_count(int jt, int64_t passing) {
  switch (jt) {
    case kLeftSemi: return passing > 0;
    case kLeftAnti: return passing == 0;
    case kInner:
    case kRightOuter: return passing;
    case kLeftOuter:
    case kFullOuter: return passing > 0 ? passing : 1;
    default: return 0;   // right semi / right anti: rows come from the build flags
  }
}

// One lane per candidate slot, a wave per 64-slot word: pass word = values AND validity (lane 0 stores it and its
// popcount), and the build row of every passing slot is flagged.
__global__ void __launch_bounds__(kBlock) filter_pass_kernel(Bits values, Bits validity, int64_t total,
                                                             const int64_t* cand_right, uint8_t* build_hit,
                                                             uint64_t* pass_bits, int64_t* prefix) {
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t base = int64_t(blockIdx.x) * kBlock; base < total; base += stride) {
    const int64_t j = base + threadIdx.x;
    const int64_t w = j >> 6;                    // wave-uniform: kBlock and base are multiples of 64
    if ((w << 6) >= total) continue;             // the whole wave is past the end
    const uint64_t word = load_word(values, w) & load_word(validity, w);
    if (build_hit != nullptr && j < total && ((word >> (j & 63)) & 1)) build_hit[cand_right[j]] = 1;
    if (lane_id() == 0) {
      pass_bits[w] = word;
      prefix[w] = __popcll(word);
    }
  }
}

__global__ void filter_count_kernel(const int64_t* offsets, int64_t n, const uint64_t* pass_bits, const int64_t* prefix,
                                    int jt, uint8_t* probe_hit, int64_t* counts) {
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kBlock) {
    const int64_t passing = passing_before(pass_bits, prefix, offsets[i + 1]) - passing_before(pass_bits, prefix, offsets[i]);
    if (probe_hit != nullptr) probe_hit[i] = passing > 0;
    counts[i] = filtered_row_count(jt, passing);
  }
}

// One lane per candidate slot: a passing slot's pair goes to its final place.  cand_left[j] is the slot's probe row.
__global__ void __launch_bounds__(kBlock) filter_compact_kernel(const uint64_t* pass_bits, const int64_t* prefix,
                                                                int64_t total, const int64_t* offsets,
                                                                const int64_t* new_offsets, const int64_t* cand_left,
                                                                const int64_t* cand_right, int64_t* out_left,
                                                                int64_t* out_right) {
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t j = int64_t(blockIdx.x) * kBlock + threadIdx.x; j < total; j += stride) {
    if (!((pass_bits[j >> 6] >> (j & 63)) & 1)) continue;
    const int64_t row = cand_left[j];
    const int64_t dst = new_offsets[row] + passing_before(pass_bits, prefix, j) - passing_before(pass_bits, prefix, offsets[row]);
    out_left[dst] = row;
    out_right[dst] = cand_right[j];
  }
}

// One lane per probe row (left / full outer): a row without a passing pair owns one slot, (row, null).  The null right
// index is written as -1 and turned into (0, bit clear) by the validity kernel below.
__global__ void filter_unmatched_kernel(const int64_t* offsets, const int64_t* new_offsets, int64_t n,
                                        const uint64_t* pass_bits, const int64_t* prefix, int64_t* out_left,
                                        int64_t* out_right) {
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kBlock) {
    if (passing_before(pass_bits, prefix, offsets[i + 1]) != passing_before(pass_bits, prefix, offsets[i])) continue;
    const int64_t dst = new_offsets[i];
    out_left[dst] = i;
    out_right[dst] = -1;
  }
}

// Validity of the right indices: bit d = out_right[d] >= 0, one ballot word per wave; the -1 marks become 0.
__global__ void __launch_bounds__(kBlock) right_validity_kernel(int64_t* out_right, int64_t n, uint64_t* out_bits) {
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t base = int64_t(blockIdx.x) * kBlock; base < n; base += stride) {
    const int64_t d = base + threadIdx.x;
    bool valid = false;
    if (d < n) {
      valid = out_right[d] >= 0;
      if (!valid) out_right[d] = 0;
    }
    const uint64_t word = __ballot(valid);
    if (lane_id() == 0 && (d >> 6) < ((n + 63) >> 6)) out_bits[d >> 6] = word;
  }
}

// bit i = (flags[i] != 0) == (want_set != 0); one ballot word per wave.
__global__ void __launch_bounds__(kBlock) flags_to_mask_kernel(const uint8_t* flags, int64_t n, int want_set, uint64_t* out) {
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t base = int64_t(blockIdx.x) * kBlock; base < n; base += stride) {
    const int64_t i = base + threadIdx.x;
    const bool hit = i < n && (flags[i] != 0) == (want_set != 0);
    const uint64_t word = __ballot(hit);
    if (lane_id() == 0 && (i >> 6) < ((n + 63) >> 6)) out[i >> 6] = word;
  }
}

int check_join_type(int jt, const char* what) {
  if (jt < kLeftSemi || jt > kFullOuter) {
    set_error("%s: join type %d is not an arrow::acero::JoinType (0 .. 7)", what, jt);
    return ARX_INVALID;
  }
  return ARX_OK;
}

}  // namespace

}  // namespace arx

using namespace arx;

extern "C" {

size_t arx_hash_join_workspace_bytes(int64_t length) { return length < 0 ? 0 : scan_ws_bytes(length); }

int arx_hash_join_key_validity(const ArxSpan* columns, int num_columns, int64_t length, void* out_bits, void* stream) {
  if (length < 0 || num_columns < 0 || (num_columns > 0 && columns == nullptr) || (length > 0 && out_bits == nullptr)) {
    set_error("hash join key validity: NULL argument or negative length");
    return ARX_INVALID;
  }
  hipStream_t st = as_stream(stream);
  const int64_t words = (length + 63) >> 6;
  if (words == 0) return ARX_OK;
  int first = 1;
  for (int c = 0; c < num_columns; ++c) {
    if (columns[c].length != length) {
      set_error("hash join key validity: column %d has %lld rows, expected %lld", c, (long long)columns[c].length,
                (long long)length);
      return ARX_INVALID;
    }
    if (columns[c].validity == nullptr || columns[c].null_count == 0) continue;
    const Bits b = make_bits(columns[c].validity, columns[c].offset, length);
    hipLaunchKernelGGL(key_validity_kernel, dim3(grid_for(words)), dim3(kBlock), 0, st, b, words, first,
                       static_cast<uint64_t*>(out_bits));
    ARX_CHECK_LAUNCH("key_validity_kernel");
    first = 0;
  }
  if (first) ARX_HIP(hipMemsetAsync(out_bits, 0xFF, size_t(words) * 8, st));
  return ARX_OK;
}

int arx_hash_join_bool_key(const ArxSpan* values, uint8_t* out, void* stream) {
  if (values == nullptr || (values->length > 0 && (values->data == nullptr || out == nullptr))) {
    set_error("hash join bool key: NULL argument");
    return ARX_INVALID;
  }
  if (values->length == 0) return ARX_OK;
  const Bits bits = make_bits(values->data, values->offset, values->length);
  hipLaunchKernelGGL(bool_key_kernel, dim3(grid_for(values->length)), dim3(kBlock), 0, as_stream(stream), bits,
                     values->length, out);
  ARX_CHECK_LAUNCH("bool_key_kernel");
  return ARX_OK;
}

int arx_hash_join_group_offsets(const uint32_t* build_ids, const void* build_valid, int64_t num_build_rows,
                                int64_t num_groups, int64_t* out_group_offsets, void* ws, size_t ws_bytes, void* stream) {
  if (num_build_rows < 0 || num_groups < 0 || num_groups > num_build_rows || out_group_offsets == nullptr ||
      (num_build_rows > 0 && build_ids == nullptr)) {
    set_error("hash join group offsets: NULL argument or num_groups outside 0 .. num_build_rows");
    return ARX_INVALID;
  }
  hipStream_t st = as_stream(stream);
  ARX_HIP(hipMemsetAsync(out_group_offsets, 0, size_t(num_groups + 1) * 8, st));
  if (num_build_rows > 0 && num_groups > 0) {
    hipLaunchKernelGGL(group_histogram_kernel, dim3(grid_for(num_build_rows)), dim3(kBlock), 0, st, build_ids,
                       static_cast<const uint64_t*>(build_valid), num_build_rows, num_groups,
                       reinterpret_cast<unsigned long long*>(out_group_offsets));
    ARX_CHECK_LAUNCH("group_histogram_kernel");
  }
  return scan_in_place(out_group_offsets, num_groups, ws, ws_bytes, st);
}

int arx_hash_join_probe_count(const uint32_t* probe_ids, const void* probe_valid, int64_t num_probe_rows,
                              const int64_t* group_offsets, int64_t num_groups, int join_type, uint8_t* matched,
                              int64_t max_output, int64_t* out_offsets, void* ws, size_t ws_bytes, int64_t* out_total,
                              void* stream) {
  if (const int rc = check_join_type(join_type, "hash join probe count"); rc != ARX_OK) return rc;
  if (num_probe_rows < 0 || num_groups < 0 || group_offsets == nullptr || out_offsets == nullptr || out_total == nullptr ||
      (num_probe_rows > 0 && probe_ids == nullptr)) {
    set_error("hash join probe count: NULL argument or negative length");
    return ARX_INVALID;
  }
  hipStream_t st = as_stream(stream);
  if (num_probe_rows > 0) {
    hipLaunchKernelGGL(probe_count_kernel, dim3(grid_for(num_probe_rows)), dim3(kBlock), 0, st, probe_ids,
                       static_cast<const uint64_t*>(probe_valid), num_probe_rows, group_offsets, num_groups, join_type,
                       matched, out_offsets);
    ARX_CHECK_LAUNCH("probe_count_kernel");
  }
  if (const int rc = scan_in_place(out_offsets, num_probe_rows, ws, ws_bytes, st); rc != ARX_OK) return rc;
  uint64_t header[2] = {0, 0};
  ARX_HIP(hipMemcpyAsync(header, ws, sizeof(header), hipMemcpyDeviceToHost, st));
  ARX_HIP(hipStreamSynchronize(st));
  if (header[1] != 0) {
    set_error("hash join: the output would have more than 2^63 - 1 rows");
    return ARX_CAPACITY_ERROR;
  }
  *out_total = static_cast<int64_t>(header[0]);
  if (max_output >= 0 && *out_total > max_output) {
    set_error("hash join: the output would have %lld rows, more than the %lld that can be allocated",
              (long long)*out_total, (long long)max_output);
    return ARX_CAPACITY_ERROR;
  }
  return ARX_OK;
}

int arx_hash_join_expand(const int64_t* offsets, const uint32_t* probe_ids, const void* probe_valid, int64_t num_probe_rows,
                         const int64_t* group_offsets, const uint64_t* build_rows_by_group, int join_type, int64_t total,
                         int64_t* out_left, int64_t* out_right, void* out_right_validity, void* stream) {
  if (const int rc = check_join_type(join_type, "hash join expand"); rc != ARX_OK) return rc;
  const bool right = join_type == kInner || join_type == kLeftOuter || join_type == kRightOuter || join_type == kFullOuter;
  if (total < 0 || num_probe_rows < 0 || (total > 0 && (num_probe_rows == 0 || offsets == nullptr || probe_ids == nullptr ||
                                                        out_left == nullptr)) ||
      (total > 0 && right && (out_right == nullptr || group_offsets == nullptr || build_rows_by_group == nullptr))) {
    set_error("hash join expand: NULL argument or a total without probe rows");
    return ARX_INVALID;
  }
  if (total == 0) return ARX_OK;
  const int64_t tiles = ceil_div(total, kExpandSlots);
  const unsigned grid = unsigned(tiles < int64_t(kMaxGrid) ? tiles : int64_t(kMaxGrid));   // the kernel strides over the rest
  hipLaunchKernelGGL(expand_kernel, dim3(grid), dim3(kBlock), 0, as_stream(stream), offsets, probe_ids,
                     static_cast<const uint64_t*>(probe_valid), num_probe_rows, group_offsets, build_rows_by_group,
                     join_type, total, out_left, right ? out_right : nullptr,
                     right ? static_cast<uint64_t*>(out_right_validity) : nullptr);
  ARX_CHECK_LAUNCH("expand_kernel");
  return ARX_OK;
}

int arx_hash_join_build_mask(const uint32_t* build_ids, const void* build_valid, int64_t num_build_rows,
                             const uint8_t* matched, int want_matched, void* out_bits, void* stream) {
  if (num_build_rows < 0 || (num_build_rows > 0 && (build_ids == nullptr || matched == nullptr || out_bits == nullptr))) {
    set_error("hash join build mask: NULL argument or negative length");
    return ARX_INVALID;
  }
  if (num_build_rows == 0) return ARX_OK;
  hipLaunchKernelGGL(build_mask_kernel, dim3(grid_for(num_build_rows)), dim3(kBlock), 0, as_stream(stream), build_ids,
                     static_cast<const uint64_t*>(build_valid), num_build_rows, matched, want_matched,
                     static_cast<uint64_t*>(out_bits));
  ARX_CHECK_LAUNCH("build_mask_kernel");
  return ARX_OK;
}

int arx_hash_join_append_build_rows(const uint64_t* build_rows, int64_t count, int64_t start, int64_t* out_left,
                                    void* out_left_validity, int64_t* out_right, void* out_right_validity, void* stream) {
  if (count < 0 || start < 0 || (count > 0 && (build_rows == nullptr || out_left == nullptr || out_right == nullptr))) {
    set_error("hash join append build rows: NULL argument or negative length");
    return ARX_INVALID;
  }
  if (count == 0) return ARX_OK;
  const int64_t lanes = count > (start + count + 63) / 64 ? count : (start + count + 63) / 64;
  hipLaunchKernelGGL(append_build_rows_kernel, dim3(grid_for(lanes)), dim3(kBlock), 0, as_stream(stream), build_rows, count,
                     start, out_left, static_cast<uint64_t*>(out_left_validity), out_right,
                     static_cast<uint64_t*>(out_right_validity));
  ARX_CHECK_LAUNCH("append_build_rows_kernel");
  return ARX_OK;
}

int arx_hash_join_filter_count(const ArxSpan* pass, const int64_t* offsets, const int64_t* cand_right,
                               int64_t num_probe_rows, int join_type, uint8_t* build_hit, uint8_t* probe_hit,
                               int64_t max_output, void* out_pass_bits, int64_t* out_pass_prefix, int64_t* out_new_offsets,
                               void* ws, size_t ws_bytes, int64_t* out_total, void* stream) {
  if (const int rc = check_join_type(join_type, "hash join filter count"); rc != ARX_OK) return rc;
  if (pass == nullptr || pass->length < 0 || num_probe_rows < 0 || out_pass_prefix == nullptr || out_new_offsets == nullptr ||
      out_total == nullptr || (num_probe_rows > 0 && offsets == nullptr) ||
      (pass->length > 0 && (pass->data == nullptr || out_pass_bits == nullptr || num_probe_rows == 0)) ||
      (pass->length > 0 && build_hit != nullptr && cand_right == nullptr)) {
    set_error("hash join filter count: NULL argument, negative length or candidates without probe rows");
    return ARX_INVALID;
  }
  hipStream_t st = as_stream(stream);
  const int64_t total = pass->length, words = (total + 63) >> 6;
  if (total > 0) {
    const Bits values = make_bits(pass->data, pass->offset, total);
    const Bits validity = make_bits(pass->null_count == 0 ? nullptr : pass->validity, pass->offset, total);
    hipLaunchKernelGGL(filter_pass_kernel, dim3(grid_for(total)), dim3(kBlock), 0, st, values, validity, total, cand_right,
                       build_hit, static_cast<uint64_t*>(out_pass_bits), out_pass_prefix);
    ARX_CHECK_LAUNCH("filter_pass_kernel");
  }
  if (const int rc = scan_in_place(out_pass_prefix, words, ws, ws_bytes, st); rc != ARX_OK) return rc;
  if (num_probe_rows > 0) {
    hipLaunchKernelGGL(filter_count_kernel, dim3(grid_for(num_probe_rows)), dim3(kBlock), 0, st, offsets, num_probe_rows,
                       static_cast<const uint64_t*>(out_pass_bits), out_pass_prefix, join_type, probe_hit, out_new_offsets);
    ARX_CHECK_LAUNCH("filter_count_kernel");
  }
  if (const int rc = scan_in_place(out_new_offsets, num_probe_rows, ws, ws_bytes, st); rc != ARX_OK) return rc;
  uint64_t header[2] = {0, 0};
  ARX_HIP(hipMemcpyAsync(header, ws, sizeof(header), hipMemcpyDeviceToHost, st));
  ARX_HIP(hipStreamSynchronize(st));
  *out_total = static_cast<int64_t>(header[0]);   // at most T + num_probe_rows: no overflow to report
  if (max_output >= 0 && *out_total > max_output) {
    set_error("hash join: the filtered output would have %lld rows, more than the %lld that can be allocated",
              (long long)*out_total, (long long)max_output);
    return ARX_CAPACITY_ERROR;
  }
  return ARX_OK;
}

int arx_hash_join_filter_compact(const void* pass_bits, const int64_t* pass_prefix, int64_t num_candidates,
                                 const int64_t* offsets, const int64_t* new_offsets, int64_t num_probe_rows,
                                 const int64_t* cand_left, const int64_t* cand_right, int join_type, int64_t total,
                                 int64_t* out_left, int64_t* out_right, void* out_right_validity, void* stream) {
  if (const int rc = check_join_type(join_type, "hash join filter compact"); rc != ARX_OK) return rc;
  if (join_type != kInner && join_type != kLeftOuter && join_type != kRightOuter && join_type != kFullOuter) {
    set_error("hash join filter compact: join type %d emits no pairs (semi / anti rows come from the flags)", join_type);
    return ARX_INVALID;
  }
  const bool outer = join_type == kLeftOuter || join_type == kFullOuter;
  if (num_candidates < 0 || num_probe_rows < 0 || total < 0 ||
      (total > 0 && (out_left == nullptr || out_right == nullptr || offsets == nullptr || new_offsets == nullptr ||
                     pass_prefix == nullptr)) ||
      (total > 0 && outer && out_right_validity == nullptr) ||
      (num_candidates > 0 && (pass_bits == nullptr || cand_left == nullptr || cand_right == nullptr))) {
    set_error("hash join filter compact: NULL argument or negative length");
    return ARX_INVALID;
  }
  if (total == 0) return ARX_OK;
  hipStream_t st = as_stream(stream);
  if (num_candidates > 0) {
    hipLaunchKernelGGL(filter_compact_kernel, dim3(grid_for(num_candidates)), dim3(kBlock), 0, st,
                       static_cast<const uint64_t*>(pass_bits), pass_prefix, num_candidates, offsets, new_offsets, cand_left,
                       cand_right, out_left, out_right);
    ARX_CHECK_LAUNCH("filter_compact_kernel");
  }
  if (outer) {
    hipLaunchKernelGGL(filter_unmatched_kernel, dim3(grid_for(num_probe_rows)), dim3(kBlock), 0, st, offsets, new_offsets,
                       num_probe_rows, static_cast<const uint64_t*>(pass_bits), pass_prefix, out_left, out_right);
    ARX_CHECK_LAUNCH("filter_unmatched_kernel");
    hipLaunchKernelGGL(right_validity_kernel, dim3(grid_for(total)), dim3(kBlock), 0, st, out_right, total,
                       static_cast<uint64_t*>(out_right_validity));
    ARX_CHECK_LAUNCH("right_validity_kernel");
  }
  return ARX_OK;
}

int arx_hash_join_flags_to_mask(const uint8_t* flags, int64_t length, int want_set, void* out_bits, void* stream) {
  if (length < 0 || (length > 0 && (flags == nullptr || out_bits == nullptr))) {
    set_error("hash join flags to mask: NULL argument or negative length");
    return ARX_INVALID;
  }
  if (length == 0) return ARX_OK;
  hipLaunchKernelGGL(flags_to_mask_kernel, dim3(grid_for(length)), dim3(kBlock), 0, as_stream(stream), flags, length,
                     want_set, static_cast<uint64_t*>(out_bits));
  ARX_CHECK_LAUNCH("flags_to_mask_kernel");
  return ARX_OK;
}

}  // extern "C"

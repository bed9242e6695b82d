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

}  // extern "C"

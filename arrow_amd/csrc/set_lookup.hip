// Set lookup: is_in / index_in against a value set held on the device — the reference's SetLookupState
// (compute/kernels/scalar_set_lookup.cc): a memo table of the set's distinct values, each with the index of its first
// occurrence, plus "the set holds a null" and that null's index; then one probe per input row.
//
// Table (the state): an open-addressing hash table of `cap` slots, cap a power of two >= 2 x the set's length, so it is
// at most half full and every probe sequence (linear, +1) ends at an empty slot.  Per slot a 32-bit INDEX (the first
// occurrence; 0xFFFFFFFF = empty — the key is never read to decide emptiness, so no key value can pass for an empty
// slot) and the KEY: the value's bits for fixed widths 1 / 2 / 4 / 8 / 16 (compared by bits like the reference's
// physical-type memo tables: NaN payloads and -0.0 / 0.0 stay apart), a 64-bit hash of the bytes for utf8 / binary
// (a hash match is confirmed on the bytes of the set's value).
//
// Build: round by round without any wait inside a kernel.  `prepare` gives every valid set value its home slot (nulls
// go to the header with atomicMin).  `claim`: every value still looking tries atomicCAS(empty -> its index) on its
// current slot and the winner writes the key.  `settle` (a separate launch, so every key of the round is written): a
// loser whose slot holds an equal key folds its index in with atomicMin and stops; any other loser moves one slot on.
// Values with equal keys walk the same slots, so they all stop at the one slot the first of them claimed.
//
// Probe: one lane per row, a __ballot per wave for the 64-bit output word (is_in: the result; index_in: the validity of
// the int32 indices).  A table of at most kSetLdsBudget bytes is copied into LDS by every workgroup, which then walks its
// share of the rows (small-set form); a larger one is probed where it lies and stays in L2 / the MALL (global form).
#include "arx_common.h"
#include "string_hash.h"

#include <algorithm>
#include <atomic>
#include <cstring>

namespace arx {

namespace {

constexpr uint32_t kSlotEmpty = 0xFFFFFFFFu;   // index field of an empty slot; set indices are < 2^30
constexpr int64_t kMaxSetLength = int64_t(1) << 30;   // 2 x the length must fit the 32-bit slot count (2^31 slots)
constexpr uint32_t kSmallSlots = 256;          // first LDS tier: sets of up to 128 values (IN lists)
constexpr int kSetLdsBudget = 64 * 1024;       // second LDS tier: the largest table that still leaves 2 workgroups per CU
constexpr unsigned kProbeGroups = 2048;        // persistent probe grid: 8 workgroups per CU of the 256-CU part

std::atomic<int64_t> g_set_lookup_lds_probes{0}, g_set_lookup_global_probes{0};

struct SetHeader {
  uint32_t null_index;    // smallest index of a null in the set, kSlotEmpty if there is none
  uint32_t pending;       // build: values still looking for their slot after this round
  uint32_t first_false;   // boolean sets: smallest index of a false / true
  uint32_t first_true;
};
constexpr size_t kHeaderBytes = 256;

struct K16 {
  uint64_t lo, hi;
};
template <int KW> struct KeyOf;
template <> struct KeyOf<1> { using T = uint8_t; };
template <> struct KeyOf<2> { using T = uint16_t; };
template <> struct KeyOf<4> { using T = uint32_t; };
template <> struct KeyOf<8> { using T = uint64_t; };
template <> struct KeyOf<16> { using T = K16; };

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 33;
  x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33;
  x *= 0xC4CEB9FE1A85EC53ull;
  return x ^ (x >> 33);
}
template <typename T>
__device__ __forceinline__ uint32_t key_home(T k) { return static_cast<uint32_t>(mix64(static_cast<uint64_t>(k))); }
__device__ __forceinline__ uint32_t key_home(K16 k) { return static_cast<uint32_t>(mix64(k.lo ^ mix64(k.hi ^ 0x9E3779B97F4A7C15ull))); }
template <typename T>
__device__ __forceinline__ bool key_eq(T a, T b) { return a == b; }
__device__ __forceinline__ bool key_eq(K16 a, K16 b) { return a.lo == b.lo && a.hi == b.hi; }

static inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// slots of a set of n values (0 <= n <= kMaxSetLength): a power of two >= 2 n (at least 64), at most 2^31
static inline uint32_t set_capacity(int64_t n) {
  uint64_t cap = 64;
  while (cap < static_cast<uint64_t>(2 * std::min(std::max<int64_t>(n, 0), kMaxSetLength))) cap <<= 1;
  return static_cast<uint32_t>(cap);
}

// key bytes per slot: the width for fixed widths, 8 (the hash) for binary (kw < 0); boolean sets (kw 0) have no table
struct SetLayout {
  uint32_t cap;
  size_t off_idx, off_key, off_pos, off_hash, total;
};
static SetLayout set_layout(int64_t n, int kw) {
  SetLayout l{};
  l.cap = set_capacity(n);
  if (kw == 0) {
    l.total = kHeaderBytes;
    return l;
  }
  const size_t kb = kw < 0 ? 8 : static_cast<size_t>(kw);
  l.off_idx = kHeaderBytes;
  l.off_key = align256(l.off_idx + static_cast<size_t>(l.cap) * 4);
  l.off_pos = align256(l.off_key + static_cast<size_t>(l.cap) * kb);
  l.off_hash = align256(l.off_pos + static_cast<size_t>(n) * 4);
  l.total = align256(l.off_hash + (kw < 0 ? static_cast<size_t>(n) * 8 : 0));
  return l;
}

// the largest table (power-of-two slots) of key width kb that fits kSetLdsBudget
constexpr uint32_t lds_slots(int kb) {
  uint32_t c = 1;
  while (static_cast<size_t>(c) * 2 * (4 + kb) <= static_cast<size_t>(kSetLdsBudget)) c *= 2;
  return c;
}

static inline unsigned build_grid(int64_t n) {
  return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, 16384)));
}
static inline unsigned probe_grid(int64_t n) {
  return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, kProbeGroups)));
}

// ---------------------------------------------------------------- strings
template <typename O>
__device__ __forceinline__ uint64_t string_hash(const O* offsets, const uint8_t* data, int64_t i, uint64_t keep) {
  const int64_t start = offsets[i];
  const int64_t len = static_cast<int64_t>(offsets[i + 1]) - start;
  uint64_t acc = 0;
  for (int64_t pos = 0; pos < len; pos += 8) acc ^= string_word_mix(string_word(data, start, len, pos), pos >> 3);
  return string_hash_finish(acc, len) & keep;
}

template <typename OA, typename OB>
__device__ __forceinline__ bool string_eq(const OA* oa, const uint8_t* da, int64_t a, const OB* ob, const uint8_t* db, int64_t b) {
  const int64_t sa = oa[a], sb = ob[b];
  const int64_t len = static_cast<int64_t>(oa[a + 1]) - sa;
  if (static_cast<int64_t>(ob[b + 1]) - sb != len) return false;
  for (int64_t pos = 0; pos < len; pos += 8) {
    if (string_word(da, sa, len, pos) != string_word(db, sb, len, pos)) return false;
  }
  return true;
}

// ---------------------------------------------------------------- build: fixed widths
template <typename T>
__global__ __launch_bounds__(kBlock) void set_build_prepare_kernel(SetHeader* hdr, Bits valid, const T* __restrict__ values,
                                                                   int64_t n, uint32_t mask, uint32_t* __restrict__ pos) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * kBlock) {
    if ((load_word(valid, i >> 6) >> (i & 63)) & 1) {
      pos[i] = key_home(values[i]) & mask;
    } else {
      atomicMin(&hdr->null_index, static_cast<uint32_t>(i));
      pos[i] = kSlotEmpty;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void set_build_claim_kernel(uint32_t* __restrict__ idx, T* __restrict__ key,
                                                                 const T* __restrict__ values, int64_t n, uint32_t* __restrict__ pos) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * kBlock) {
    const uint32_t p = pos[i];
    if (p == kSlotEmpty) continue;
    if (atomicCAS(&idx[p], kSlotEmpty, static_cast<uint32_t>(i)) == kSlotEmpty) {
      key[p] = values[i];
      pos[i] = kSlotEmpty;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void set_build_settle_kernel(SetHeader* hdr, uint32_t* __restrict__ idx, const T* __restrict__ key,
                                                                  const T* __restrict__ values, int64_t n, uint32_t mask,
                                                                  uint32_t* __restrict__ pos) {
  uint32_t pending = 0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * kBlock) {
    const uint32_t p = pos[i];
    if (p == kSlotEmpty) continue;
    if (key_eq(key[p], values[i])) {
      atomicMin(&idx[p], static_cast<uint32_t>(i));
      pos[i] = kSlotEmpty;
    } else {
      pos[i] = (p + 1) & mask;
      ++pending;
    }
  }
  if (pending != 0) atomicAdd(&hdr->pending, pending);
}

// ---------------------------------------------------------------- build: binary (the key is the hash of the bytes)
template <typename O>
__global__ __launch_bounds__(kBlock) void set_build_prepare_binary_kernel(SetHeader* hdr, Bits valid, const O* __restrict__ offsets,
                                                                          const uint8_t* __restrict__ data, int64_t n, uint64_t keep,
                                                                          uint32_t mask, uint32_t* __restrict__ pos,
                                                                          uint64_t* __restrict__ hashes) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * kBlock) {
    if ((load_word(valid, i >> 6) >> (i & 63)) & 1) {
      const uint64_t h = string_hash(offsets, data, i, keep);
      hashes[i] = h;
      pos[i] = key_home(h) & mask;
    } else {
      atomicMin(&hdr->null_index, static_cast<uint32_t>(i));
      pos[i] = kSlotEmpty;
    }
  }
}

template <typename O>
__global__ __launch_bounds__(kBlock) void set_build_settle_binary_kernel(SetHeader* hdr, uint32_t* __restrict__ idx,
                                                                         const uint64_t* __restrict__ key, const O* __restrict__ offsets,
                                                                         const uint8_t* __restrict__ data, const uint64_t* __restrict__ hashes,
                                                                         int64_t n, uint32_t mask, uint32_t* __restrict__ pos) {
  uint32_t pending = 0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * kBlock) {
    const uint32_t p = pos[i];
    if (p == kSlotEmpty) continue;
    // idx[p] may be lowered concurrently, but every index it can hold names a value with these very bytes
    if (key[p] == hashes[i] && string_eq(offsets, data, static_cast<int64_t>(idx[p]), offsets, data, i)) {
      atomicMin(&idx[p], static_cast<uint32_t>(i));
      pos[i] = kSlotEmpty;
    } else {
      pos[i] = (p + 1) & mask;
      ++pending;
    }
  }
  if (pending != 0) atomicAdd(&hdr->pending, pending);
}

// ---------------------------------------------------------------- build: boolean (first false, first true, first null)
__global__ __launch_bounds__(kBlock) void set_build_boolean_kernel(SetHeader* hdr, Bits valid, Bits bits, int64_t n) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * kBlock) {
    const uint32_t u = static_cast<uint32_t>(i);
    if (!((load_word(valid, i >> 6) >> (i & 63)) & 1)) {
      atomicMin(&hdr->null_index, u);
    } else if ((load_word(bits, i >> 6) >> (i & 63)) & 1) {
      atomicMin(&hdr->first_true, u);
    } else {
      atomicMin(&hdr->first_false, u);
    }
  }
}

// ---------------------------------------------------------------- probe
template <typename T>
__device__ __forceinline__ uint32_t set_find(const uint32_t* idx, const T* key, uint32_t mask, T k) {
  uint32_t p = key_home(k) & mask;
  while (true) {
    const uint32_t id = idx[p];
    if (id == kSlotEmpty || key_eq(key[p], k)) return id;
    p = (p + 1) & mask;
  }
}

template <typename OS, typename OI>
__device__ __forceinline__ uint32_t set_find_binary(const uint32_t* idx, const uint64_t* key, uint32_t mask, uint64_t h,
                                                    const OS* s_off, const uint8_t* s_data, const OI* offsets,
                                                    const uint8_t* data, int64_t row) {
  uint32_t p = key_home(h) & mask;
  while (true) {
    const uint32_t id = idx[p];
    if (id == kSlotEmpty) return id;
    if (key[p] == h && string_eq(offsets, data, row, s_off, s_data, static_cast<int64_t>(id))) return id;
    p = (p + 1) & mask;
  }
}

// One row per lane; rows [base, base + 256) per workgroup step, so a wave's 64 rows are one output word.  The ballot of
// "found" is the is_in word, or the validity word of index_in (a miss is null there).  A null row is looked up as the
// set's null unless skip_nulls.
__device__ __forceinline__ void emit_row(uint32_t hit, int64_t row, int64_t n, uint64_t* __restrict__ out_bits,
                                         int32_t* __restrict__ out_index) {
  const uint64_t m = __ballot(hit != kSlotEmpty);
  if (row < n) {
    if (out_index != nullptr) out_index[row] = hit == kSlotEmpty ? 0 : static_cast<int32_t>(hit);
    if (lane_id() == 0) out_bits[row >> 6] = m;
  }
}

template <int KW, uint32_t LCAP>
__global__ __launch_bounds__(kBlock) void set_probe_kernel(const SetHeader* __restrict__ hdr, const uint32_t* __restrict__ g_idx,
                                                           const typename KeyOf<KW>::T* __restrict__ g_key, uint32_t cap, Bits valid,
                                                           const typename KeyOf<KW>::T* __restrict__ values, int64_t n,
                                                           int skip_nulls, uint64_t* __restrict__ out_bits,
                                                           int32_t* __restrict__ out_index) {
  using T = typename KeyOf<KW>::T;
  __shared__ uint32_t s_idx[LCAP > 0 ? LCAP : 1];
  __shared__ T s_key[LCAP > 0 ? LCAP : 1];
  if constexpr (LCAP > 0) {
    for (uint32_t i = threadIdx.x; i < cap; i += kBlock) {
      s_idx[i] = g_idx[i];
      s_key[i] = g_key[i];
    }
    __syncthreads();
  }
  const uint32_t mask = cap - 1;
  const uint32_t null_hit = skip_nulls ? kSlotEmpty : hdr->null_index;
  const int lane = lane_id();
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kBlock; base < n; base += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t row = base + threadIdx.x;
    const bool ok = (load_word(valid, row >> 6) >> lane) & 1;   // 0 past the end
    uint32_t hit = null_hit;
    if (ok) {
      if constexpr (LCAP > 0) {
        hit = set_find(s_idx, s_key, mask, values[row]);
      } else {
        hit = set_find(g_idx, g_key, mask, values[row]);
      }
    }
    emit_row(row < n ? hit : kSlotEmpty, row, n, out_bits, out_index);
  }
}

template <typename OS, typename OI, uint32_t LCAP>
__global__ __launch_bounds__(kBlock) void set_probe_binary_kernel(const SetHeader* __restrict__ hdr, const uint32_t* __restrict__ g_idx,
                                                                  const uint64_t* __restrict__ g_key, uint32_t cap,
                                                                  const OS* __restrict__ s_off, const uint8_t* __restrict__ s_data,
                                                                  Bits valid, const OI* __restrict__ offsets,
                                                                  const uint8_t* __restrict__ data, int64_t n, uint64_t keep,
                                                                  int skip_nulls, uint64_t* __restrict__ out_bits,
                                                                  int32_t* __restrict__ out_index) {
  __shared__ uint32_t s_idx[LCAP > 0 ? LCAP : 1];
  __shared__ uint64_t s_key[LCAP > 0 ? LCAP : 1];
  if constexpr (LCAP > 0) {
    for (uint32_t i = threadIdx.x; i < cap; i += kBlock) {
      s_idx[i] = g_idx[i];
      s_key[i] = g_key[i];
    }
    __syncthreads();
  }
  const uint32_t mask = cap - 1;
  const uint32_t null_hit = skip_nulls ? kSlotEmpty : hdr->null_index;
  const int lane = lane_id();
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kBlock; base < n; base += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t row = base + threadIdx.x;
    const bool ok = (load_word(valid, row >> 6) >> lane) & 1;
    uint32_t hit = null_hit;
    if (ok) {
      const uint64_t h = string_hash(offsets, data, row, keep);
      if constexpr (LCAP > 0) {
        hit = set_find_binary(s_idx, s_key, mask, h, s_off, s_data, offsets, data, row);
      } else {
        hit = set_find_binary(g_idx, g_key, mask, h, s_off, s_data, offsets, data, row);
      }
    }
    emit_row(row < n ? hit : kSlotEmpty, row, n, out_bits, out_index);
  }
}

__global__ __launch_bounds__(kBlock) void set_probe_boolean_kernel(const SetHeader* __restrict__ hdr, Bits valid, Bits bits, int64_t n,
                                                                   int skip_nulls, uint64_t* __restrict__ out_bits,
                                                                   int32_t* __restrict__ out_index) {
  const uint32_t null_hit = skip_nulls ? kSlotEmpty : hdr->null_index;
  const uint32_t first_true = hdr->first_true, first_false = hdr->first_false;
  const int lane = lane_id();
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kBlock; base < n; base += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t row = base + threadIdx.x;
    const bool ok = (load_word(valid, row >> 6) >> lane) & 1;
    const bool v = (load_word(bits, row >> 6) >> lane) & 1;
    const uint32_t hit = ok ? (v ? first_true : first_false) : null_hit;
    emit_row(row < n ? hit : kSlotEmpty, row, n, out_bits, out_index);
  }
}

// ---------------------------------------------------------------- host side
int check_set_length(int64_t n, const char* what) {
  if (n < 0 || n > kMaxSetLength) {
    set_error("%s: the value set's length %lld is outside 0 .. 2^30 (its table has at most 2^31 slots)", what,
              static_cast<long long>(n));
    return ARX_CAPACITY_ERROR;
  }
  return ARX_OK;
}

// the header and the empty table (every field of both is "none" = 0xFF bytes)
int set_reset(void* state, const SetLayout& l, int kw, hipStream_t st) {
  const size_t bytes = kw == 0 ? kHeaderBytes : l.off_idx + static_cast<size_t>(l.cap) * 4;
  ARX_HIP(hipMemsetAsync(state, 0xFF, bytes, st));
  return ARX_OK;
}

// the rounds of claim + settle until every value has its slot (at most the longest probe sequence of the table)
template <typename Claim, typename Settle>
int set_build_rounds(SetHeader* hdr, int64_t n, hipStream_t st, Claim claim, Settle settle) {
  for (int64_t round = 0;; ++round) {
    claim();
    ARX_CHECK_LAUNCH("set_build_claim_kernel");
    ARX_HIP(hipMemsetAsync(&hdr->pending, 0, 4, st));
    settle();
    ARX_CHECK_LAUNCH("set_build_settle_kernel");
    uint32_t pending = 0;
    ARX_HIP(hipMemcpyAsync(&pending, &hdr->pending, 4, hipMemcpyDeviceToHost, st));
    ARX_HIP(hipStreamSynchronize(st));
    if (pending == 0) return ARX_OK;
    if (round > 2 * n + 2) {
      set_error("set lookup build: %u values found no slot", pending);
      return ARX_INVALID;
    }
  }
}

template <int KW>
int build_fixed(void* state, const ArxSpan* set, hipStream_t st) {
  using T = typename KeyOf<KW>::T;
  const int64_t n = set->length;
  const SetLayout l = set_layout(n, KW);
  if (const int rc = set_reset(state, l, KW, st); rc != ARX_OK) return rc;
  if (n == 0) return ARX_OK;
  uint8_t* base = static_cast<uint8_t*>(state);
  auto* hdr = reinterpret_cast<SetHeader*>(base);
  auto* idx = reinterpret_cast<uint32_t*>(base + l.off_idx);
  auto* key = reinterpret_cast<T*>(base + l.off_key);
  auto* pos = reinterpret_cast<uint32_t*>(base + l.off_pos);
  const T* values = static_cast<const T*>(set->data) + set->offset;
  const Bits valid = make_bits(set->null_count == 0 ? nullptr : set->validity, set->offset, n);
  const unsigned g = build_grid(n);
  const uint32_t mask = l.cap - 1;
  hipLaunchKernelGGL(set_build_prepare_kernel<T>, dim3(g), dim3(kBlock), 0, st, hdr, valid, values, n, mask, pos);
  ARX_CHECK_LAUNCH("set_build_prepare_kernel");
  return set_build_rounds(
      hdr, n, st, [&] { hipLaunchKernelGGL(set_build_claim_kernel<T>, dim3(g), dim3(kBlock), 0, st, idx, key, values, n, pos); },
      [&] { hipLaunchKernelGGL(set_build_settle_kernel<T>, dim3(g), dim3(kBlock), 0, st, hdr, idx, key, values, n, mask, pos); });
}

template <typename O>
int build_binary(void* state, const ArxBinarySpan* set, uint64_t keep, hipStream_t st) {
  const int64_t n = set->length;
  const SetLayout l = set_layout(n, -1);
  if (const int rc = set_reset(state, l, -1, st); rc != ARX_OK) return rc;
  if (n == 0) return ARX_OK;
  uint8_t* base = static_cast<uint8_t*>(state);
  auto* hdr = reinterpret_cast<SetHeader*>(base);
  auto* idx = reinterpret_cast<uint32_t*>(base + l.off_idx);
  auto* key = reinterpret_cast<uint64_t*>(base + l.off_key);
  auto* pos = reinterpret_cast<uint32_t*>(base + l.off_pos);
  auto* hashes = reinterpret_cast<uint64_t*>(base + l.off_hash);
  const O* offsets = reinterpret_cast<const O*>(set->offsets) + set->offset;
  const uint8_t* data = static_cast<const uint8_t*>(set->data);
  const Bits valid = make_bits(set->null_count == 0 ? nullptr : set->validity, set->offset, n);
  const unsigned g = build_grid(n);
  const uint32_t mask = l.cap - 1;
  hipLaunchKernelGGL(set_build_prepare_binary_kernel<O>, dim3(g), dim3(kBlock), 0, st, hdr, valid, offsets, data, n, keep, mask, pos,
                     hashes);
  ARX_CHECK_LAUNCH("set_build_prepare_binary_kernel");
  return set_build_rounds(
      hdr, n, st, [&] { hipLaunchKernelGGL(set_build_claim_kernel<uint64_t>, dim3(g), dim3(kBlock), 0, st, idx, key, hashes, n, pos); },
      [&] {
        hipLaunchKernelGGL(set_build_settle_binary_kernel<O>, dim3(g), dim3(kBlock), 0, st, hdr, idx, key, offsets, data, hashes, n,
                           mask, pos);
      });
}

template <int KW>
int probe_fixed(const void* state, int64_t set_length, const ArxSpan* values, int skip_nulls, void* out_bits, int32_t* out_index,
                hipStream_t st) {
  using T = typename KeyOf<KW>::T;
  const SetLayout l = set_layout(set_length, KW);
  const uint8_t* base = static_cast<const uint8_t*>(state);
  const auto* hdr = reinterpret_cast<const SetHeader*>(base);
  const auto* idx = reinterpret_cast<const uint32_t*>(base + l.off_idx);
  const auto* key = reinterpret_cast<const T*>(base + l.off_key);
  const int64_t n = values->length;
  const T* v = static_cast<const T*>(values->data) + values->offset;
  const Bits valid = make_bits(values->null_count == 0 ? nullptr : values->validity, values->offset, n);
  auto* out = static_cast<uint64_t*>(out_bits);
  constexpr uint32_t kLarge = lds_slots(KW);
  const dim3 g(probe_grid(n));
  if (l.cap <= kSmallSlots) {
    hipLaunchKernelGGL((set_probe_kernel<KW, kSmallSlots>), g, dim3(kBlock), 0, st, hdr, idx, key, l.cap, valid, v, n, skip_nulls, out,
                       out_index);
    g_set_lookup_lds_probes.fetch_add(1, std::memory_order_relaxed);
  } else if (l.cap <= kLarge) {
    hipLaunchKernelGGL((set_probe_kernel<KW, kLarge>), g, dim3(kBlock), 0, st, hdr, idx, key, l.cap, valid, v, n, skip_nulls, out,
                       out_index);
    g_set_lookup_lds_probes.fetch_add(1, std::memory_order_relaxed);
  } else {
    hipLaunchKernelGGL((set_probe_kernel<KW, 0>), g, dim3(kBlock), 0, st, hdr, idx, key, l.cap, valid, v, n, skip_nulls, out, out_index);
    g_set_lookup_global_probes.fetch_add(1, std::memory_order_relaxed);
  }
  ARX_CHECK_LAUNCH("set_probe_kernel");
  return ARX_OK;
}

template <typename OS, typename OI>
int probe_binary(const void* state, const ArxBinarySpan* set, const ArxBinarySpan* values, uint64_t keep, int skip_nulls,
                 void* out_bits, int32_t* out_index, hipStream_t st) {
  const SetLayout l = set_layout(set->length, -1);
  const uint8_t* base = static_cast<const uint8_t*>(state);
  const auto* hdr = reinterpret_cast<const SetHeader*>(base);
  const auto* idx = reinterpret_cast<const uint32_t*>(base + l.off_idx);
  const auto* key = reinterpret_cast<const uint64_t*>(base + l.off_key);
  const OS* s_off = reinterpret_cast<const OS*>(set->offsets) + set->offset;
  const auto* s_data = static_cast<const uint8_t*>(set->data);
  const int64_t n = values->length;
  const OI* offsets = reinterpret_cast<const OI*>(values->offsets) + values->offset;
  const auto* data = static_cast<const uint8_t*>(values->data);
  const Bits valid = make_bits(values->null_count == 0 ? nullptr : values->validity, values->offset, n);
  auto* out = static_cast<uint64_t*>(out_bits);
  constexpr uint32_t kLarge = lds_slots(8);
  const dim3 g(probe_grid(n));
  if (l.cap <= kSmallSlots) {
    hipLaunchKernelGGL((set_probe_binary_kernel<OS, OI, kSmallSlots>), g, dim3(kBlock), 0, st, hdr, idx, key, l.cap, s_off, s_data,
                       valid, offsets, data, n, keep, skip_nulls, out, out_index);
    g_set_lookup_lds_probes.fetch_add(1, std::memory_order_relaxed);
  } else if (l.cap <= kLarge) {
    hipLaunchKernelGGL((set_probe_binary_kernel<OS, OI, kLarge>), g, dim3(kBlock), 0, st, hdr, idx, key, l.cap, s_off, s_data, valid,
                       offsets, data, n, keep, skip_nulls, out, out_index);
    g_set_lookup_lds_probes.fetch_add(1, std::memory_order_relaxed);
  } else {
    hipLaunchKernelGGL((set_probe_binary_kernel<OS, OI, 0>), g, dim3(kBlock), 0, st, hdr, idx, key, l.cap, s_off, s_data, valid,
                       offsets, data, n, keep, skip_nulls, out, out_index);
    g_set_lookup_global_probes.fetch_add(1, std::memory_order_relaxed);
  }
  ARX_CHECK_LAUNCH("set_probe_binary_kernel");
  return ARX_OK;
}

int probe_any(const void* state, int64_t set_length, int key_width, const ArxSpan* values, int skip_nulls, void* out_bits,
              int32_t* out_index, void* stream) {
  if (state == nullptr || values == nullptr) {
    set_error("set lookup: NULL state or values");
    return ARX_INVALID;
  }
  if (const int rc = check_set_length(set_length, "set lookup"); rc != ARX_OK) return rc;
  if (values->length <= 0) return ARX_OK;
  if (values->data == nullptr || out_bits == nullptr) {
    set_error("set lookup: NULL buffer");
    return ARX_INVALID;
  }
  hipStream_t st = as_stream(stream);
  switch (key_width) {
    case 0: {
      const int64_t n = values->length;
      const Bits valid = make_bits(values->null_count == 0 ? nullptr : values->validity, values->offset, n);
      const Bits bits = make_bits(values->data, values->offset, n);
      hipLaunchKernelGGL(set_probe_boolean_kernel, dim3(probe_grid(n)), dim3(kBlock), 0, st, static_cast<const SetHeader*>(state), valid,
                         bits, n, skip_nulls, static_cast<uint64_t*>(out_bits), out_index);
      ARX_CHECK_LAUNCH("set_probe_boolean_kernel");
      return ARX_OK;
    }
    case 1: return probe_fixed<1>(state, set_length, values, skip_nulls, out_bits, out_index, st);
    case 2: return probe_fixed<2>(state, set_length, values, skip_nulls, out_bits, out_index, st);
    case 4: return probe_fixed<4>(state, set_length, values, skip_nulls, out_bits, out_index, st);
    case 8: return probe_fixed<8>(state, set_length, values, skip_nulls, out_bits, out_index, st);
    case 16: return probe_fixed<16>(state, set_length, values, skip_nulls, out_bits, out_index, st);
    default:
      set_error("set lookup: key width %d is not 0 (boolean), 1, 2, 4, 8 or 16", key_width);
      return ARX_INVALID;
  }
}

int probe_binary_any(const void* state, const ArxBinarySpan* set, int set_offset_width, int hash_bits, const ArxBinarySpan* values,
                     int offset_width, int skip_nulls, void* out_bits, int32_t* out_index, void* stream) {
  if (state == nullptr || set == nullptr || values == nullptr) {
    set_error("set lookup binary: NULL state, value set or values");
    return ARX_INVALID;
  }
  if ((set_offset_width != 4 && set_offset_width != 8) || (offset_width != 4 && offset_width != 8) || hash_bits < 1 || hash_bits > 64) {
    set_error("set lookup binary: offset widths must be 4 or 8 and hash_bits 1 .. 64");
    return ARX_INVALID;
  }
  if (const int rc = check_set_length(set->length, "set lookup binary"); rc != ARX_OK) return rc;
  if (values->length <= 0) return ARX_OK;
  if (values->offsets == nullptr || out_bits == nullptr) {
    set_error("set lookup binary: NULL buffer");
    return ARX_INVALID;
  }
  const uint64_t keep = hash_bits >= 64 ? ~uint64_t(0) : ((uint64_t(1) << hash_bits) - 1);
  hipStream_t st = as_stream(stream);
  if (set_offset_width == 4) {
    return offset_width == 4 ? probe_binary<int32_t, int32_t>(state, set, values, keep, skip_nulls, out_bits, out_index, st)
                             : probe_binary<int32_t, int64_t>(state, set, values, keep, skip_nulls, out_bits, out_index, st);
  }
  return offset_width == 4 ? probe_binary<int64_t, int32_t>(state, set, values, keep, skip_nulls, out_bits, out_index, st)
                           : probe_binary<int64_t, int64_t>(state, set, values, keep, skip_nulls, out_bits, out_index, st);
}

}  // namespace

static const CounterRow kSetLookupCounters[] = {
    {"set_lookup_lds_probes", &g_set_lookup_lds_probes},
    {"set_lookup_global_probes", &g_set_lookup_global_probes},
};
CounterTable set_lookup_counters() { return counter_table(kSetLookupCounters); }

}  // namespace arx

using namespace arx;

extern "C" {

size_t arx_set_lookup_state_bytes(int64_t set_length, int key_width) {
  if (set_length < 0 || set_length > kMaxSetLength) return 0;   // no table: build refuses the length
  return set_layout(set_length, key_width).total;
}

int arx_set_lookup_build(void* state, const ArxSpan* value_set, int key_width, void* stream) {
  if (state == nullptr || value_set == nullptr) {
    set_error("set lookup build: NULL state or value set");
    return ARX_INVALID;
  }
  if (const int rc = check_set_length(value_set->length, "set lookup build"); rc != ARX_OK) return rc;
  if (value_set->length > 0 && value_set->data == nullptr) {
    set_error("set lookup build: NULL values buffer");
    return ARX_INVALID;
  }
  hipStream_t st = as_stream(stream);
  switch (key_width) {
    case 0: {
      const int64_t n = value_set->length;
      if (const int rc = set_reset(state, set_layout(n, 0), 0, st); rc != ARX_OK) return rc;
      if (n > 0) {
        const Bits valid = make_bits(value_set->null_count == 0 ? nullptr : value_set->validity, value_set->offset, n);
        const Bits bits = make_bits(value_set->data, value_set->offset, n);
        hipLaunchKernelGGL(set_build_boolean_kernel, dim3(build_grid(n)), dim3(kBlock), 0, st, static_cast<SetHeader*>(state), valid,
                           bits, n);
        ARX_CHECK_LAUNCH("set_build_boolean_kernel");
      }
      ARX_HIP(hipStreamSynchronize(st));
      return ARX_OK;
    }
    case 1: return build_fixed<1>(state, value_set, st);
    case 2: return build_fixed<2>(state, value_set, st);
    case 4: return build_fixed<4>(state, value_set, st);
    case 8: return build_fixed<8>(state, value_set, st);
    case 16: return build_fixed<16>(state, value_set, st);
    default:
      set_error("set lookup build: key width %d is not 0 (boolean), 1, 2, 4, 8 or 16", key_width);
      return ARX_INVALID;
  }
}

int arx_set_lookup_build_binary(void* state, const ArxBinarySpan* value_set, int offset_width, int hash_bits, void* stream) {
  if (state == nullptr || value_set == nullptr || (offset_width != 4 && offset_width != 8) || hash_bits < 1 || hash_bits > 64) {
    set_error("set lookup build binary: NULL argument, offset width not 4 / 8 or hash_bits outside 1 .. 64");
    return ARX_INVALID;
  }
  if (const int rc = check_set_length(value_set->length, "set lookup build binary"); rc != ARX_OK) return rc;
  if (value_set->length > 0 && value_set->offsets == nullptr) {
    set_error("set lookup build binary: NULL offsets buffer");
    return ARX_INVALID;
  }
  const uint64_t keep = hash_bits >= 64 ? ~uint64_t(0) : ((uint64_t(1) << hash_bits) - 1);
  hipStream_t st = as_stream(stream);
  return offset_width == 4 ? build_binary<int32_t>(state, value_set, keep, st) : build_binary<int64_t>(state, value_set, keep, st);
}

int arx_set_lookup_is_in(const void* state, int64_t set_length, int key_width, const ArxSpan* values, int skip_nulls, void* out_bits,
                         void* stream) {
  return probe_any(state, set_length, key_width, values, skip_nulls, out_bits, nullptr, stream);
}

int arx_set_lookup_index_in(const void* state, int64_t set_length, int key_width, const ArxSpan* values, int skip_nulls,
                            int32_t* out_index, void* out_validity, void* stream) {
  if (values != nullptr && values->length > 0 && out_index == nullptr) {
    set_error("set lookup index_in: NULL output");
    return ARX_INVALID;
  }
  return probe_any(state, set_length, key_width, values, skip_nulls, out_validity, out_index, stream);
}

int arx_set_lookup_is_in_binary(const void* state, const ArxBinarySpan* value_set, int set_offset_width, int hash_bits,
                                const ArxBinarySpan* values, int offset_width, int skip_nulls, void* out_bits, void* stream) {
  return probe_binary_any(state, value_set, set_offset_width, hash_bits, values, offset_width, skip_nulls, out_bits, nullptr, stream);
}

int arx_set_lookup_index_in_binary(const void* state, const ArxBinarySpan* value_set, int set_offset_width, int hash_bits,
                                   const ArxBinarySpan* values, int offset_width, int skip_nulls, int32_t* out_index,
                                   void* out_validity, void* stream) {
  if (values != nullptr && values->length > 0 && out_index == nullptr) {
    set_error("set lookup index_in binary: NULL output");
    return ARX_INVALID;
  }
  return probe_binary_any(state, value_set, set_offset_width, hash_bits, values, offset_width, skip_nulls, out_validity, out_index,
                          stream);
}

}  // extern "C"

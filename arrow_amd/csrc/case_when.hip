// case_when(conds, v_0 .. v_{k-1} [, else]) for one fixed-width (or boolean) type on gfx950 — what a SQL CASE with more
// than one WHEN lowers to.
//
// What it restates (semantics only):
//   CaseWhenFunctor / ExecArrayCaseWhen   cpp/src/arrow/compute/kernels/scalar_if_else.cc   (fixed-width types, boolean)
// Row i takes v_j[i] of the first j whose cond is true and valid (a null cond is false); a row no cond takes comes from
// the else, or is null without one.  The result's validity is the chosen operand's.  On the 64-row words of the bitmaps:
// remaining = ~0; take_j = remaining & c_j & cv_j; remaining &= ~take_j; the else takes what remains;
// valid = OR_j (take_j & vv_j).  A null result slot is written as zero (as if_else.hip does), so two builds' outputs
// compare byte for byte.  Every value: an array, a valid scalar or a null scalar.
//
// Shape, widths 8 and 16: a wave takes kCaseWhenWords consecutive words (256 rows), lane = row within a word.  The bitmap
// words are wave-uniform (scalar loads).  The walk over the branches only picks, per row, WHERE its value comes from (a
// pointer into the chosen stream, or the chosen scalar); after the walk a lane issues its one load per row, all of them
// before the first store.  So a row costs one value load whatever k is, a stream none of a word's rows takes is not
// touched (nor are the parts of a stream whose rows went elsewhere), and the walk stops once no row of the wave's words
// remains: later cond bitmaps are not read either.
// Widths 1, 2 and 4 (case_when_packed_kernel): a lane takes 8 / W consecutive rows, so a load or store moves 8 bytes a
// lane; the rows of a lane may come from different branches, so the walk loads a branch's 8 bytes where the lane takes any
// of them (kCaseWhenPackedSteps such loads in flight per branch) and merges them under a byte mask.
// Booleans: 64 rows per lane with bit operations.  The operand descriptors travel by value in the kernel arguments.
#include "arx_common.h"

#include <algorithm>

namespace arx {

// rows one wave takes at a time (tests/test_case_when.py: ROWS_PER_WAVE): 64 x kCaseWhenWords at widths 8 and 16,
// 64 x (8 / W) x kCaseWhenPackedSteps at widths 1, 2 and 4
constexpr int kCaseWhenWords = 4;
constexpr int kCaseWhenPackedSteps = 4;
constexpr int64_t kCaseWhenMaxBlocks = 1 << 20;   // workgroups of a launch (a wave strides over what is left)
constexpr int kCaseWhenMaxValues = ARX_CASE_WHEN_MAX_CONDS + 1;

static std::atomic<int64_t> g_case_when_launches{0};          // case_when_kernel<T>: widths 8 and 16
static std::atomic<int64_t> g_case_when_packed_launches{0};   // case_when_packed_kernel<T>: widths 1, 2 and 4
static std::atomic<int64_t> g_case_when_bool_launches{0};     // case_when_bool_kernel
static constexpr CounterRow kCaseWhenCounters[] = {
    {"case_when_launches", &g_case_when_launches},
    {"case_when_packed_launches", &g_case_when_packed_launches},
    {"case_when_bool_launches", &g_case_when_bool_launches},
};
CounterTable case_when_counters() { return counter_table(kCaseWhenCounters); }

struct CaseWhenU128 {
  uint64_t lo, hi;
};

enum { kCaseWhenArray = 0, kCaseWhenScalar = 1, kCaseWhenNull = 2 };

// one value of a fixed-width call: `data` is logical element 0 (arrays), `valid` the array's bitmap (NULL base: none)
template <typename T>
struct CaseWhenValue {
  const T* data;
  T scalar;
  Bits valid;
  int kind;
};
// a boolean value: `data` the value bits of an array
struct CaseWhenBoolValue {
  Bits data;
  Bits valid;
  int kind;
  int scalar;
};
// the whole call, by value in the kernel arguments (2.2 KB at width 16)
template <class Value>
struct CaseWhenArgs {
  Bits cond[ARX_CASE_WHEN_MAX_CONDS];
  Bits cond_valid[ARX_CASE_WHEN_MAX_CONDS];
  Value value[kCaseWhenMaxValues];   // value[num_conds]: the else, when num_values == num_conds + 1
  int num_conds;
  int num_values;
};

// the rows of word w branch j takes out of `remaining` (the else: all of them)
template <class Args>
__device__ __forceinline__ uint64_t case_when_take(const Args& a, int j, int64_t w, uint64_t remaining) {
  if (j >= a.num_conds) return remaining;
  return remaining & load_word(a.cond[j], w) & load_word(a.cond_valid[j], w);
}
__device__ __forceinline__ uint64_t case_when_valid_word(const Bits& valid, int kind, int64_t w) {
  return kind == kCaseWhenNull ? 0ull : load_word(valid, w);
}
// all ones below `n`
__device__ __forceinline__ uint64_t case_when_rows_word(int64_t n, int64_t w) {
  const Bits rows{nullptr, 0, n, 0};
  return load_word(rows, w);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void case_when_kernel(CaseWhenArgs<CaseWhenValue<T>> a, int64_t n, T* __restrict__ out,
                                                           uint64_t* __restrict__ out_valid) {
  const int lane = lane_id();
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  const int64_t nwords = (n + 63) >> 6;
  const int64_t nsteps = (nwords + kCaseWhenWords - 1) / kCaseWhenWords;
  for (int64_t s = wave; s < nsteps; s += nwaves) {
    const int64_t w0 = s * kCaseWhenWords;
    uint64_t remaining[kCaseWhenWords], valid[kCaseWhenWords];   // (wave-uniform)
    const T* src[kCaseWhenWords];                                // this lane's row: the stream it comes from, or
    T v[kCaseWhenWords];                                         // the scalar it is (zero: a null slot)
#pragma unroll
    for (int k = 0; k < kCaseWhenWords; ++k) {
      remaining[k] = case_when_rows_word(n, w0 + k);   // (a word past the last one: nothing remains, nothing is stored)
      valid[k] = 0;
      src[k] = nullptr;
      v[k] = T{};
    }
    for (int j = 0; j < a.num_values; ++j) {
      const CaseWhenValue<T>& x = a.value[j];
      uint64_t left = 0;
#pragma unroll
      for (int k = 0; k < kCaseWhenWords; ++k) {
        const int64_t w = w0 + k;
        const uint64_t take = case_when_take(a, j, w, remaining[k]);
        remaining[k] &= ~take;
        left |= remaining[k];
        const uint64_t need = take & case_when_valid_word(x.valid, x.kind, w);
        valid[k] |= need;
        if ((need >> lane) & 1ull) {   // (a row below n: `remaining` starts from the rows there are)
          src[k] = x.kind == kCaseWhenArray ? x.data + ((w << 6) + lane) : nullptr;
          v[k] = x.scalar;
        }
      }
      if (left == 0) break;   // (wave-uniform) every row of the step has its value
    }
#pragma unroll
    for (int k = 0; k < kCaseWhenWords; ++k) {
      if (src[k] != nullptr) v[k] = *src[k];
    }
#pragma unroll
    for (int k = 0; k < kCaseWhenWords; ++k) {
      const int64_t w = w0 + k;
      const int64_t i = (w << 6) + lane;
      if (i < n) out[i] = v[k];
      if (lane == 0 && out_valid != nullptr && w < nwords) out_valid[w] = valid[k];
    }
  }
}

// widths 1, 2 and 4: a lane takes kV = 8 / W consecutive rows (they lie in one word: word lane / (64 / kV) of a step's kV,
// from bit (lane % (64 / kV)) * kV), as if_else_packed_kernel does.  The inputs carry their own element offsets, so their
// 8 bytes are read at any alignment; a lane whose rows straddle `n` reads and writes them one by one.
template <typename T>
__global__ __launch_bounds__(kBlock) void case_when_packed_kernel(CaseWhenArgs<CaseWhenValue<T>> a, int64_t n, T* __restrict__ out,
                                                                  uint64_t* __restrict__ out_valid) {
  constexpr int kV = 8 / static_cast<int>(sizeof(T));
  constexpr int kLanesPerWord = 64 / kV;
  constexpr int kBits = 8 * static_cast<int>(sizeof(T));
  constexpr uint64_t kElement = (uint64_t(1) << kBits) - 1;
  constexpr uint64_t kRows = (uint64_t(1) << kV) - 1;
  const int lane = lane_id();
  const int my_word = lane / kLanesPerWord;
  const int my_shift = (lane % kLanesPerWord) * kV;
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  const int64_t nwords = (n + 63) >> 6;
  const int64_t nsteps = (nwords + kV * kCaseWhenPackedSteps - 1) / (kV * kCaseWhenPackedSteps);
  for (int64_t s = wave; s < nsteps; s += nwaves) {
    uint64_t remaining[kCaseWhenPackedSteps], valid[kCaseWhenPackedSteps];   // this lane's word of each step
    uint64_t acc[kCaseWhenPackedSteps];                                      // this lane's 8 bytes of each step
#pragma unroll
    for (int k = 0; k < kCaseWhenPackedSteps; ++k) {
      remaining[k] = case_when_rows_word(n, (s * kCaseWhenPackedSteps + k) * kV + my_word);
      valid[k] = 0;
      acc[k] = 0;
    }
    for (int j = 0; j < a.num_values; ++j) {
      const CaseWhenValue<T>& x = a.value[j];
      uint64_t scalar = 0;   // the scalar, kV times over
#pragma unroll
      for (int e = 0; e < kV; ++e) scalar |= static_cast<uint64_t>(x.scalar) << (e * kBits);
      uint64_t rows[kCaseWhenPackedSteps], got[kCaseWhenPackedSteps];
      bool left = false;
#pragma unroll
      for (int k = 0; k < kCaseWhenPackedSteps; ++k) {
        const int64_t w0 = (s * kCaseWhenPackedSteps + k) * kV;
        uint64_t need = 0;
#pragma unroll
        for (int e = 0; e < kV; ++e) {   // (wave-uniform words; a lane keeps its own)
          const int64_t w = w0 + e;
          const uint64_t take = case_when_take(a, j, w, ~0ull);
          const uint64_t vw = case_when_valid_word(x.valid, x.kind, w);
          if (my_word == e) {
            const uint64_t mine = take & remaining[k];
            remaining[k] &= ~mine;
            need = mine & vw;
          }
        }
        valid[k] |= need;
        left = left || remaining[k] != 0;
        rows[k] = (need >> my_shift) & kRows;
        got[k] = scalar;
        const int64_t row0 = (w0 << 6) + lane * kV;
        if (x.kind == kCaseWhenArray && rows[k] != 0) {
          if (row0 + kV <= n) {
            __builtin_memcpy(&got[k], x.data + row0, 8);
          } else {
            got[k] = 0;
            for (int e = 0; e < kV; ++e) {
              if (row0 + e < n) got[k] |= static_cast<uint64_t>(x.data[row0 + e]) << (e * kBits);
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < kCaseWhenPackedSteps; ++k) {
        uint64_t mask = 0;
#pragma unroll
        for (int e = 0; e < kV; ++e) {
          if ((rows[k] >> e) & 1ull) mask |= kElement << (e * kBits);
        }
        acc[k] |= got[k] & mask;   // (the branches' rows are disjoint)
      }
      if (!__any(left)) break;   // every row of the wave's step has its value
    }
#pragma unroll
    for (int k = 0; k < kCaseWhenPackedSteps; ++k) {
      const int64_t w0 = (s * kCaseWhenPackedSteps + k) * kV;
      const int64_t row0 = (w0 << 6) + lane * kV;
      if (row0 + kV <= n) {
        __builtin_memcpy(out + row0, &acc[k], 8);
      } else {
        for (int e = 0; e < kV; ++e) {
          if (row0 + e < n) out[row0 + e] = static_cast<T>(acc[k] >> (e * kBits));
        }
      }
      if (lane % kLanesPerWord == 0 && out_valid != nullptr && w0 + my_word < nwords) out_valid[w0 + my_word] = valid[k];
    }
  }
}

// booleans: 64 rows per lane
__global__ __launch_bounds__(kBlock) void case_when_bool_kernel(CaseWhenArgs<CaseWhenBoolValue> a, int64_t n, uint64_t* __restrict__ out,
                                                                uint64_t* __restrict__ out_valid) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  const int64_t nwords = (n + 63) >> 6;
  for (int64_t w = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; w < nwords; w += stride) {
    uint64_t remaining = case_when_rows_word(n, w);
    uint64_t data = 0, valid = 0;
    for (int j = 0; j < a.num_values && remaining != 0; ++j) {
      const CaseWhenBoolValue& x = a.value[j];
      const uint64_t take = case_when_take(a, j, w, remaining);
      remaining &= ~take;
      const uint64_t need = take & case_when_valid_word(x.valid, x.kind, w);
      valid |= need;
      if (need != 0) data |= need & (x.kind == kCaseWhenArray ? load_word(x.data, w) : (x.scalar ? ~0ull : 0ull));
    }
    out[w] = data;
    if (out_valid != nullptr) out_valid[w] = valid;
  }
}

static int case_when_kind(const ArxOperand& o) {
  return o.span != nullptr ? kCaseWhenArray : (o.scalar != nullptr ? kCaseWhenScalar : kCaseWhenNull);
}
static bool case_when_has_bitmap(const ArxSpan* span) { return span != nullptr && span->validity != nullptr && span->null_count != 0; }
static Bits case_when_valid_bits(const ArxSpan* span, int64_t length) {
  return make_bits(case_when_has_bitmap(span) ? span->validity : nullptr, span != nullptr ? span->offset : 0, length);
}

template <class Value>
static void case_when_conds(const ArxSpan* const* conds, int num_conds, int num_values, int64_t length, CaseWhenArgs<Value>* a) {
  for (int j = 0; j < num_conds; ++j) {
    a->cond[j] = make_bits(conds[j]->data, conds[j]->offset, length);
    a->cond_valid[j] = case_when_valid_bits(conds[j], length);
  }
  a->num_conds = num_conds;
  a->num_values = num_values;
}

template <typename T>
static CaseWhenArgs<CaseWhenValue<T>> case_when_args(const ArxSpan* const* conds, int num_conds, const ArxOperand* values, int num_values,
                                                     int64_t length) {
  CaseWhenArgs<CaseWhenValue<T>> a{};
  case_when_conds(conds, num_conds, num_values, length, &a);
  for (int j = 0; j < num_values; ++j) {
    CaseWhenValue<T>& x = a.value[j];
    const ArxSpan* span = values[j].span;
    x.data = span != nullptr ? static_cast<const T*>(span->data) + span->offset : nullptr;
    x.scalar = T{};
    if (span == nullptr && values[j].scalar != nullptr) __builtin_memcpy(&x.scalar, values[j].scalar, sizeof(T));
    x.valid = case_when_valid_bits(span, length);
    x.kind = case_when_kind(values[j]);
  }
  return a;
}

extern "C" {

int arx_case_when(int byte_width, const ArxSpan* const* conds, int num_conds, const ArxOperand* values, int num_values,
                  int64_t length, void* out_data, void* out_validity, void* stream) {
  if (byte_width != 0 && byte_width != 1 && byte_width != 2 && byte_width != 4 && byte_width != 8 && byte_width != 16) {
    set_error("arx_case_when: byte_width %d (0 = boolean, 1, 2, 4, 8, 16)", byte_width);
    return ARX_INVALID;
  }
  if (num_conds < 1 || num_conds > ARX_CASE_WHEN_MAX_CONDS) {
    set_error("arx_case_when: %d conds; the device kernel takes 1 to %d", num_conds, ARX_CASE_WHEN_MAX_CONDS);
    return ARX_INVALID;
  }
  if (num_values != num_conds && num_values != num_conds + 1) {
    set_error("arx_case_when: %d values for %d conds (as many, or one more: the else)", num_values, num_conds);
    return ARX_INVALID;
  }
  if (length < 0) {
    set_error("arx_case_when: negative length %lld", static_cast<long long>(length));
    return ARX_INVALID;
  }
  if (conds == nullptr || values == nullptr) {
    set_error("arx_case_when: NULL %s", conds == nullptr ? "conds" : "values");
    return ARX_INVALID;
  }
  for (int j = 0; j < num_conds; ++j) {
    if (conds[j] == nullptr) {
      set_error("arx_case_when: NULL cond %d", j);
      return ARX_INVALID;
    }
    if (conds[j]->length != length) {
      set_error("arx_case_when: span length %lld of cond %d is not length %lld", static_cast<long long>(conds[j]->length), j,
                static_cast<long long>(length));
      return ARX_INVALID;
    }
  }
  for (int j = 0; j < num_values; ++j) {
    if (values[j].span != nullptr && values[j].span->length != length) {
      set_error("arx_case_when: span length %lld of value %d is not length %lld", static_cast<long long>(values[j].span->length), j,
                static_cast<long long>(length));
      return ARX_INVALID;
    }
    if (values[j].span != nullptr && values[j].scalar != nullptr) {
      set_error("arx_case_when: value %d is given as an array and as a scalar", j);
      return ARX_INVALID;
    }
  }
  if (length == 0) return ARX_OK;
  if (out_data == nullptr) {
    set_error("arx_case_when: NULL out_data");
    return ARX_INVALID;
  }
  for (int j = 0; j < num_conds; ++j) {
    if (conds[j]->data == nullptr) {
      set_error("arx_case_when: NULL data buffer of cond %d", j);
      return ARX_INVALID;
    }
  }
  bool may_have_nulls = num_values == num_conds;   // no else: a row no cond takes is null
  for (int j = 0; j < num_values; ++j) {
    if (values[j].span != nullptr && values[j].span->data == nullptr) {
      set_error("arx_case_when: NULL data buffer of value %d", j);
      return ARX_INVALID;
    }
    may_have_nulls = may_have_nulls || case_when_has_bitmap(values[j].span) || case_when_kind(values[j]) == kCaseWhenNull;
  }
  if (out_validity == nullptr && may_have_nulls) {
    set_error("arx_case_when: NULL out_validity, but there is no else, or a value has a validity bitmap or is a null scalar");
    return ARX_INVALID;
  }
  hipStream_t st = as_stream(stream);
  const int64_t nwords = ceil_div(length, 64);
  if (byte_width == 0) {
    CaseWhenArgs<CaseWhenBoolValue> a{};
    case_when_conds(conds, num_conds, num_values, length, &a);
    for (int j = 0; j < num_values; ++j) {
      CaseWhenBoolValue& x = a.value[j];
      const ArxSpan* span = values[j].span;
      x.data = span != nullptr ? make_bits(span->data, span->offset, length) : Bits{nullptr, 0, length, 0};
      x.valid = case_when_valid_bits(span, length);
      x.kind = case_when_kind(values[j]);
      x.scalar = x.kind == kCaseWhenScalar ? (*static_cast<const uint8_t*>(values[j].scalar) != 0) : 0;
    }
    const unsigned grid = static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(ceil_div(nwords, kBlock), 1 << 16)));
    hipLaunchKernelGGL(case_when_bool_kernel, dim3(grid), dim3(kBlock), 0, st, a, length, static_cast<uint64_t*>(out_data),
                       static_cast<uint64_t*>(out_validity));
    ARX_CHECK_LAUNCH("case_when_bool_kernel");
    g_case_when_bool_launches.fetch_add(1, std::memory_order_relaxed);
    return ARX_OK;
  }
  const bool packed = byte_width < 8;
  const int64_t nsteps = ceil_div(nwords, packed ? (8 / byte_width) * kCaseWhenPackedSteps : kCaseWhenWords);
  const unsigned grid = static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(ceil_div(nsteps, kWavesPerBlock), kCaseWhenMaxBlocks)));
#define ARX_CASE_WHEN_CASE(W, KERNEL, T)                                                                                          \
  case W:                                                                                                                         \
    hipLaunchKernelGGL((KERNEL<T>), dim3(grid), dim3(kBlock), 0, st, case_when_args<T>(conds, num_conds, values, num_values, length), \
                       length, static_cast<T*>(out_data), static_cast<uint64_t*>(out_validity));                                  \
    break;
  switch (byte_width) {
    ARX_CASE_WHEN_CASE(1, case_when_packed_kernel, uint8_t)
    ARX_CASE_WHEN_CASE(2, case_when_packed_kernel, uint16_t)
    ARX_CASE_WHEN_CASE(4, case_when_packed_kernel, uint32_t)
    ARX_CASE_WHEN_CASE(8, case_when_kernel, uint64_t)
    ARX_CASE_WHEN_CASE(16, case_when_kernel, CaseWhenU128)
  }
#undef ARX_CASE_WHEN_CASE
  ARX_CHECK_LAUNCH(packed ? "case_when_packed_kernel" : "case_when_kernel");
  (packed ? g_case_when_packed_launches : g_case_when_launches).fetch_add(1, std::memory_order_relaxed);
  return ARX_OK;
}

}  // extern "C"

}  // namespace arx

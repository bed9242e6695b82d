// min_element_wise / max_element_wise of 1 .. 32 operands of one numeric type on gfx950 — what GREATEST / LEAST and every
// clip such as max(x, 0) or min(qty, cap) lower to.
//
// What it restates (semantics only):
//   MinMaxFunctor / ScalarMinMax, Minimum / Maximum   cpp/src/arrow/compute/kernels/scalar_compare.cc, codegen_internal.h
// skip_nulls: a row is null only where every operand is null; otherwise where any operand is null.  The fold order shows
// on floats and is the reference's: the accumulator starts as the fold of all scalar operands (folded on the host into
// one scalar, the first valid one starting it) or, without a valid scalar, as the operation's "antiextreme" — the default
// quiet NaN for floats, the type's largest (min) or smallest (max) value for integers; then every valid value of the
// arrays, left to right, goes through the step Call(acc, x).  The step is std::fmin / std::fmax as the reference's build
// resolves them, and the two float widths differ (pyarrow 25.0.0 on x86-64, observed bit by bit):
//   double   isnan(acc) ? x : isnan(x) ? acc : (x < acc ? x : acc)      a tie of +0.0 and -0.0 keeps the accumulator, of
//            two NaNs the right one's bits come out — so the first valid value replaces the NaN the fold starts from
//   float    isnan(x) ? acc : isnan(acc) ? x : (acc < x ? acc : x)      a tie takes the right operand, of two NaNs the
//            accumulator stays — so a NaN result of arrays alone is the default NaN, even for one operand
// (max: > for <).  A NaN loses to every number in both.  Only comparisons and selects: no rounding anywhere, the same
// bits on the host and on the device.  Integers compare as their own signed or unsigned type.  A null result slot is
// written as zero.
//
// Shape (as unary_arith.hip): a lane moves 16 bytes of each operand per step — one global_load_dwordx4 at whatever
// alignment the span's offset leaves — and stores its E = 16 / sizeof(T) results in one store; element_wise_steps<T>()
// such loads of an operand are in flight per lane.  A wave's step covers E consecutive 64-row words; their validity words are
// wave-uniform (scalar loads) and a lane keeps the one its rows lie in; the first lane of each word stores the whole
// result word.  The lane whose rows straddle `length` goes row by row.  The operand table travels by value in the kernel
// arguments.  kValidity = false (no operand has a bitmap): values only.
#include "arx_common.h"

#include <algorithm>
#include <limits>
#include <type_traits>

namespace arx {

// 16-byte loads of one operand a lane issues before it folds them (tests/test_element_wise_min_max.py: ROWS_PER_WAVE): a
// lane holds 16 / W accumulators and as many loaded values per step, one register each, so the narrow types take fewer
template <typename T>
constexpr int element_wise_steps() { return sizeof(T) >= 4 ? 4 : (sizeof(T) == 2 ? 2 : 1); }
constexpr int64_t kElementWiseMaxBlocks = 1 << 20;   // workgroups of a launch (a wave strides over what is left)

static std::atomic<int64_t> g_element_wise_launches{0};
static constexpr CounterRow kElementWiseCounters[] = {
    {"element_wise_launches", &g_element_wise_launches},
};
CounterTable element_wise_counters() { return counter_table(kElementWiseCounters); }

// one step of the fold, Call(acc, x): host (the scalars) and device (the arrays)
template <typename T, bool kMax>
__host__ __device__ __forceinline__ T element_wise_step(T acc, T x) {
  if constexpr (std::is_same<T, float>::value) {
    if (x != x) return acc;
    if (acc != acc) return x;
    return kMax ? (acc > x ? acc : x) : (acc < x ? acc : x);
  } else {
    if constexpr (std::is_same<T, double>::value) {
      if (acc != acc) return x;
      if (x != x) return acc;
    }
    return kMax ? (x > acc ? x : acc) : (x < acc ? x : acc);
  }
}
// what the fold starts from without a valid scalar
template <typename T, bool kMax>
static T element_wise_antiextreme() {
  if constexpr (std::is_floating_point<T>::value) return std::numeric_limits<T>::quiet_NaN();
  else return kMax ? std::numeric_limits<T>::lowest() : std::numeric_limits<T>::max();
}

enum { kElementWiseNoScalar = 0, kElementWiseScalar = 1, kElementWiseNullScalar = 2 };

// the arrays of a call in argument order, and the one scalar its scalar operands fold to
template <typename T>
struct ElementWiseArgs {
  const T* data[ARX_ELEMENT_WISE_MAX_OPERANDS];   // logical element 0
  Bits valid[ARX_ELEMENT_WISE_MAX_OPERANDS];      // (NULL base: no bitmap)
  T scalar;                                       // the scalars' fold; without a valid scalar: the antiextreme
  int scalar_kind;
  int num_arrays;
  int skip_nulls;
};

template <typename T, int N>
struct alignas(16) ElementWiseVec {
  T v[N];
};

template <typename T, bool kMax, bool kValidity>
__global__ __launch_bounds__(kBlock) void element_wise_kernel(ElementWiseArgs<T> a, int64_t n, T* __restrict__ out,
                                                              uint64_t* __restrict__ out_valid) {
  constexpr int E = 16 / static_cast<int>(sizeof(T));   // rows of a lane's 16 bytes = words of a wave's step
  constexpr int kElementWiseSteps = element_wise_steps<T>();
  constexpr int kLanesPerWord = 64 / E;
  constexpr uint64_t kRows = (uint64_t(1) << E) - 1;
  const int lane = lane_id();
  const int my_word = lane / kLanesPerWord;
  const int my_shift = (lane % kLanesPerWord) * E;
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  const int64_t nwords = (n + 63) >> 6;
  const int64_t nsteps = (nwords + E * kElementWiseSteps - 1) / (E * kElementWiseSteps);
  const Bits rows_there{nullptr, 0, n, 0};
  for (int64_t s = wave; s < nsteps; s += nwaves) {
    ElementWiseVec<T, E> acc[kElementWiseSteps];
    uint64_t any[kElementWiseSteps], all[kElementWiseSteps];   // this lane's word: rows with a value so far / without a null so far
#pragma unroll
    for (int k = 0; k < kElementWiseSteps; ++k) {
      const uint64_t there = load_word(rows_there, (s * kElementWiseSteps + k) * E + my_word);
      any[k] = a.scalar_kind == kElementWiseScalar ? there : 0;
      all[k] = a.scalar_kind == kElementWiseNullScalar ? 0 : there;
#pragma unroll
      for (int e = 0; e < E; ++e) acc[k].v[e] = a.scalar;
    }
    for (int j = 0; j < a.num_arrays; ++j) {
      const T* __restrict__ in = a.data[j];
      ElementWiseVec<T, E> x[kElementWiseSteps];
      uint64_t xv[kElementWiseSteps];
#pragma unroll
      for (int k = 0; k < kElementWiseSteps; ++k) {
        const int64_t w0 = (s * kElementWiseSteps + k) * E;
        const int64_t row0 = (w0 << 6) + lane * E;
        if (row0 + E <= n) {
          __builtin_memcpy(&x[k], in + row0, 16);
        } else {
#pragma unroll
          for (int e = 0; e < E; ++e) x[k].v[e] = row0 + e < n ? in[row0 + e] : T(0);
        }
        xv[k] = load_word(rows_there, w0 + my_word);
        if constexpr (kValidity) {
          if (a.valid[j].base != nullptr) {   // (wave-uniform)
#pragma unroll
            for (int e = 0; e < E; ++e) {
              const uint64_t vw = load_word(a.valid[j], w0 + e);
              if (my_word == e) xv[k] = vw;
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < kElementWiseSteps; ++k) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const T folded = element_wise_step<T, kMax>(acc[k].v[e], x[k].v[e]);
          if constexpr (kValidity) {
            acc[k].v[e] = ((xv[k] >> (my_shift + e)) & 1ull) ? folded : acc[k].v[e];
          } else {
            acc[k].v[e] = folded;
          }
        }
        any[k] |= xv[k];
        all[k] &= xv[k];
      }
    }
#pragma unroll
    for (int k = 0; k < kElementWiseSteps; ++k) {
      const int64_t w0 = (s * kElementWiseSteps + k) * E;
      const int64_t row0 = (w0 << 6) + lane * E;
      const uint64_t valid = a.skip_nulls ? any[k] : all[k];
      if constexpr (kValidity) {
        const uint64_t mine = (valid >> my_shift) & kRows;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          if (((mine >> e) & 1ull) == 0) acc[k].v[e] = T(0);   // a null result slot: zero
        }
      }
      if (row0 + E <= n) {
        __builtin_memcpy(out + row0, &acc[k], 16);
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          if (row0 + e < n) out[row0 + e] = acc[k].v[e];
        }
      }
      if (lane % kLanesPerWord == 0 && out_valid != nullptr && w0 + my_word < nwords) out_valid[w0 + my_word] = valid;
    }
  }
}

static bool element_wise_has_bitmap(const ArxSpan* span) { return span != nullptr && span->validity != nullptr && span->null_count != 0; }

template <typename T, bool kMax>
static void element_wise_launch(hipStream_t st, int skip_nulls, const ArxOperand* operands, int num_operands, int64_t length, void* out_data,
                                void* out_validity) {
  ElementWiseArgs<T> a{};
  a.scalar = element_wise_antiextreme<T, kMax>();
  a.scalar_kind = kElementWiseNoScalar;
  a.skip_nulls = skip_nulls != 0;
  bool bitmaps = false;
  for (int j = 0; j < num_operands; ++j) {
    const ArxSpan* span = operands[j].span;
    if (span != nullptr) {
      a.data[a.num_arrays] = static_cast<const T*>(span->data) + span->offset;
      a.valid[a.num_arrays] = make_bits(element_wise_has_bitmap(span) ? span->validity : nullptr, span->offset, length);
      bitmaps = bitmaps || element_wise_has_bitmap(span);
      ++a.num_arrays;
    } else if (operands[j].scalar == nullptr) {
      if (!a.skip_nulls) a.scalar_kind = kElementWiseNullScalar;   // (under skip_nulls a null scalar is no operand)
    } else if (a.scalar_kind != kElementWiseNullScalar) {
      T x;
      __builtin_memcpy(&x, operands[j].scalar, sizeof(T));
      a.scalar = a.scalar_kind == kElementWiseScalar ? element_wise_step<T, kMax>(a.scalar, x) : x;
      a.scalar_kind = kElementWiseScalar;
    }
  }
  constexpr int E = 16 / static_cast<int>(sizeof(T));
  const int64_t nsteps = ceil_div(ceil_div(length, 64), E * element_wise_steps<T>());
  const unsigned grid = static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(ceil_div(nsteps, kWavesPerBlock), kElementWiseMaxBlocks)));
  // the values-only form folds every row of every operand: right when nothing can be null, and no validity is asked for
  const bool validity = bitmaps || a.scalar_kind == kElementWiseNullScalar || a.num_arrays == 0 || out_validity != nullptr;
  if (validity) {
    hipLaunchKernelGGL((element_wise_kernel<T, kMax, true>), dim3(grid), dim3(kBlock), 0, st, a, length, static_cast<T*>(out_data),
                       static_cast<uint64_t*>(out_validity));
  } else {
    hipLaunchKernelGGL((element_wise_kernel<T, kMax, false>), dim3(grid), dim3(kBlock), 0, st, a, length, static_cast<T*>(out_data),
                       static_cast<uint64_t*>(out_validity));
  }
}

#define ARX_ELEMENT_WISE_ALL_TYPES(CASE)                                                                                \
  CASE(ARX_NUM_INT8, int8_t) CASE(ARX_NUM_UINT8, uint8_t) CASE(ARX_NUM_INT16, int16_t) CASE(ARX_NUM_UINT16, uint16_t)  \
  CASE(ARX_NUM_INT32, int32_t) CASE(ARX_NUM_UINT32, uint32_t) CASE(ARX_NUM_INT64, int64_t) CASE(ARX_NUM_UINT64, uint64_t) \
  CASE(ARX_NUM_FLOAT32, float) CASE(ARX_NUM_FLOAT64, double)

extern "C" {

int arx_min_max_element_wise(int num_type, int op, int skip_nulls, const ArxOperand* operands, int num_operands, int64_t length,
                             void* out_data, void* out_validity, void* stream) {
  if (num_type < ARX_NUM_INT8 || num_type > ARX_NUM_FLOAT64) {
    set_error("arx_min_max_element_wise: numeric type %d (ARX_NUM_INT8 .. ARX_NUM_FLOAT64)", num_type);
    return ARX_INVALID;
  }
  if (op != ARX_ELEMENT_WISE_MIN && op != ARX_ELEMENT_WISE_MAX) {
    set_error("arx_min_max_element_wise: op %d (ARX_ELEMENT_WISE_MIN, ARX_ELEMENT_WISE_MAX)", op);
    return ARX_INVALID;
  }
  if (num_operands < 1 || num_operands > ARX_ELEMENT_WISE_MAX_OPERANDS) {
    set_error("arx_min_max_element_wise: %d operands; the device kernel takes 1 to %d", num_operands, ARX_ELEMENT_WISE_MAX_OPERANDS);
    return ARX_INVALID;
  }
  if (length < 0) {
    set_error("arx_min_max_element_wise: negative length %lld", static_cast<long long>(length));
    return ARX_INVALID;
  }
  if (operands == nullptr) {
    set_error("arx_min_max_element_wise: NULL operands");
    return ARX_INVALID;
  }
  bool any_nullable = false, all_nullable = true;
  for (int j = 0; j < num_operands; ++j) {
    const ArxSpan* span = operands[j].span;
    if (span != nullptr && span->length != length) {
      set_error("arx_min_max_element_wise: span length %lld of operand %d is not length %lld", static_cast<long long>(span->length), j,
                static_cast<long long>(length));
      return ARX_INVALID;
    }
    if (span != nullptr && operands[j].scalar != nullptr) {
      set_error("arx_min_max_element_wise: operand %d is given as an array and as a scalar", j);
      return ARX_INVALID;
    }
    const bool nullable = span != nullptr ? element_wise_has_bitmap(span) : operands[j].scalar == nullptr;
    any_nullable = any_nullable || nullable;
    all_nullable = all_nullable && nullable;
  }
  if (length == 0) return ARX_OK;
  if (out_data == nullptr) {
    set_error("arx_min_max_element_wise: NULL out_data");
    return ARX_INVALID;
  }
  for (int j = 0; j < num_operands; ++j) {
    if (operands[j].span != nullptr && operands[j].span->data == nullptr) {
      set_error("arx_min_max_element_wise: NULL data buffer of operand %d", j);
      return ARX_INVALID;
    }
  }
  if (out_validity == nullptr && (skip_nulls != 0 ? all_nullable : any_nullable)) {
    set_error("arx_min_max_element_wise: NULL out_validity, but %s", skip_nulls != 0
                  ? "every operand has a validity bitmap or is a null scalar"
                  : "an operand has a validity bitmap or is a null scalar");
    return ARX_INVALID;
  }
  hipStream_t st = as_stream(stream);
  switch (num_type) {
#define ARX_ELEMENT_WISE_CASE(CODE, T)                                                                                     \
  case CODE:                                                                                                               \
    if (op == ARX_ELEMENT_WISE_MAX) element_wise_launch<T, true>(st, skip_nulls, operands, num_operands, length, out_data, out_validity); \
    else element_wise_launch<T, false>(st, skip_nulls, operands, num_operands, length, out_data, out_validity);             \
    break;
    ARX_ELEMENT_WISE_ALL_TYPES(ARX_ELEMENT_WISE_CASE)
#undef ARX_ELEMENT_WISE_CASE
  }
  ARX_CHECK_LAUNCH("element_wise_kernel");
  g_element_wise_launches.fetch_add(1, std::memory_order_relaxed);
  return ARX_OK;
}

}  // extern "C"

#undef ARX_ELEMENT_WISE_ALL_TYPES

}  // namespace arx

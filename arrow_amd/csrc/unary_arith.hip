// One-operand arithmetic on gfx950: negate, abs (+ _checked), sign, floor, ceil, trunc, round and round_to_multiple of
// the ten numeric types — what `-x`, `abs(a - b)`, `floor(x / 10)` and `round(price * (1 - discount), 2)` lower to.
//
// What it restates (semantics only):
//   Negate / NegateChecked / AbsoluteValue / AbsoluteValueChecked / Sign   cpp/src/arrow/compute/kernels/base_arithmetic_internal.h
//   Floor / Ceil / Trunc, Round / RoundToMultiple and the ten RoundModes   cpp/src/arrow/compute/kernels/scalar_round.cc
// Unchecked integer negate / abs wrap in the type's width (abs(int8 -128) == -128, negate(uint8 1) == 255); the checked
// forms fail on the signed minimum.  sign of an integer is int8, of a float the same float (sign(+-0.0) == +0.0, a NaN
// stays the NaN it is).  Rounding follows the reference operation by operation:
//   floats    rv = x * p (ndigits > 0) or x / p; frac = rv - floor(rv); frac == 0 keeps x; a half mode off a tie rounds half
//             away from zero, anything else by the mode's own rule; back through / p or * p; a result that is not finite
//             fails the row.  p = pow10(|ndigits|) or the multiple, made on the host.  These are exactly the IEEE
//             operations of the reference, so contraction is OFF for this file (an FMA of x * p - floor(rv) gives other
//             bits) and every division is the correctly rounded `/`.
//   integers  rem = v % m (C truncation); rem == 0 keeps v; otherwise towards zero (v - rem) or away from it (+- m) by the
//             mode; a result outside the type fails the row.  m = 10^-ndigits or the multiple.  The 64-bit `%` by the
//             uniform runtime m is the compiler's software division (DESIGN.md 4.25 has the measurement).
// A failing row is reported the way arx_divide_numeric does: *errors keeps 1 + the LAST failing valid row (the reference
// overwrites its Status slot by slot); null rows are computed like any other — their bytes are whatever they are — but
// never fail.  The result's validity is the caller's business (a bitmap copy): these kernels write values only.
// Memory: a lane moves 16 bytes of input per step (one global_load_dwordx4 at whatever alignment the span's offset
// leaves) and stores its 16 / sizeof(T) results in one store, kUnarySteps steps in flight per lane; the lane whose rows
// straddle `length` goes row by row.  Plain loads and stores, as in temporal.hip.
#include "arx_common.h"

#include <string.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <type_traits>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace arx {

constexpr int kUnarySteps = 4;                  // 16-byte loads a lane issues before its first result
constexpr int64_t kUnaryMaxBlocks = 1 << 20;    // workgroups of a launch (a workgroup strides over what is left)

static std::atomic<int64_t> g_unary_arith_launches{0};   // negate .. trunc
static std::atomic<int64_t> g_round_launches{0};         // round, round_to_multiple
static constexpr CounterRow kUnaryCounters[] = {
    {"unary_arith_launches", &g_unary_arith_launches},
    {"round_launches", &g_round_launches},
};
CounterTable unary_arith_counters() { return counter_table(kUnaryCounters); }

// ---------------------------------------------------------------- float helpers: the same operations on host and device
template <typename T> struct FloatBits;
template <> struct FloatBits<float> { using type = uint32_t; static constexpr uint32_t kSign = 0x80000000u; };
template <> struct FloatBits<double> { using type = uint64_t; static constexpr uint64_t kSign = 0x8000000000000000ull; };

template <typename T>
__host__ __device__ __forceinline__ T flip_sign(T v) {
  using B = typename FloatBits<T>::type;
  return __builtin_bit_cast(T, static_cast<B>(__builtin_bit_cast(B, v) ^ FloatBits<T>::kSign));
}
template <typename T>
__host__ __device__ __forceinline__ T clear_sign(T v) {
  using B = typename FloatBits<T>::type;
  return __builtin_bit_cast(T, static_cast<B>(__builtin_bit_cast(B, v) & ~FloatBits<T>::kSign));
}
template <typename T>
__host__ __device__ __forceinline__ bool sign_bit(T v) {
  using B = typename FloatBits<T>::type;
  return (__builtin_bit_cast(B, v) & FloatBits<T>::kSign) != 0;
}
__host__ __device__ __forceinline__ float fl_floor(float v) { return __builtin_floorf(v); }
__host__ __device__ __forceinline__ double fl_floor(double v) { return __builtin_floor(v); }
__host__ __device__ __forceinline__ float fl_ceil(float v) { return __builtin_ceilf(v); }
__host__ __device__ __forceinline__ double fl_ceil(double v) { return __builtin_ceil(v); }
__host__ __device__ __forceinline__ float fl_trunc(float v) { return __builtin_truncf(v); }
__host__ __device__ __forceinline__ double fl_trunc(double v) { return __builtin_trunc(v); }
// std::round: half away from zero.  v - trunc(v) is exact, and so is the step of one (|trunc(v)| < 2^52 when it is taken)
template <typename T>
__host__ __device__ __forceinline__ T round_half_away(T v) {
  const T t = fl_trunc(v);
  const T d = clear_sign(static_cast<T>(v - t));
  if (!(d >= T(0.5))) return t;
  return sign_bit(v) ? static_cast<T>(t - T(1)) : static_cast<T>(t + T(1));
}

// ---------------------------------------------------------------- the operations, one row each
// Every functor: `Out` and operator()(T v, bool* fail); *fail is only ever set, and only by a functor with kCanFail.
template <typename T, bool CHECKED>
struct NegateOp {
  using Out = T;
  static constexpr bool kCanFail = CHECKED && std::is_integral<T>::value;
  __device__ __forceinline__ T operator()(T v, bool* fail) const {
    if constexpr (std::is_integral<T>::value) {
      using U = typename std::make_unsigned<T>::type;
      if constexpr (kCanFail) {
        if (v == std::numeric_limits<T>::min()) *fail = true;
      }
      return static_cast<T>(static_cast<U>(U(0) - static_cast<U>(v)));
    } else {
      return flip_sign(v);
    }
  }
};

template <typename T, bool CHECKED>
struct AbsOp {
  using Out = T;
  static constexpr bool kCanFail = CHECKED && std::is_integral<T>::value && std::is_signed<T>::value;
  __device__ __forceinline__ T operator()(T v, bool* fail) const {
    if constexpr (std::is_floating_point<T>::value) {
      return clear_sign(v);
    } else if constexpr (std::is_signed<T>::value) {
      using U = typename std::make_unsigned<T>::type;
      if constexpr (kCanFail) {
        if (v == std::numeric_limits<T>::min()) *fail = true;
      }
      return v < 0 ? static_cast<T>(static_cast<U>(U(0) - static_cast<U>(v))) : v;
    } else {
      return v;
    }
  }
};

template <typename T>
struct SignOp {
  using Out = typename std::conditional<std::is_integral<T>::value, int8_t, T>::type;
  static constexpr bool kCanFail = false;
  __device__ __forceinline__ Out operator()(T v, bool*) const {
    if constexpr (std::is_floating_point<T>::value) {
      if (v != v) return v;
      return v == T(0) ? T(0) : (sign_bit(v) ? T(-1) : T(1));
    } else {
      return static_cast<int8_t>((v > T(0) ? 1 : 0) - (v < T(0) ? 1 : 0));
    }
  }
};

template <typename T, int OP>   // ARX_UNARY_FLOOR / _CEIL / _TRUNC
struct FloorOp {
  using Out = T;
  static constexpr bool kCanFail = false;
  __device__ __forceinline__ T operator()(T v, bool*) const {
    if constexpr (OP == ARX_UNARY_FLOOR) return fl_floor(v);
    else if constexpr (OP == ARX_UNARY_CEIL) return fl_ceil(v);
    else return fl_trunc(v);
  }
};

// UP: ndigits > 0 (scale up, round, scale down); otherwise divide first — ndigits <= 0 and every round_to_multiple
template <typename T, int MODE, bool UP>
struct RoundFloatOp {
  using Out = T;
  static constexpr bool kCanFail = true;
  T p;
  __device__ __forceinline__ T operator()(T x, bool* fail) const {
    if (!__builtin_isfinite(x)) return x;
    const T rv = UP ? static_cast<T>(x * p) : static_cast<T>(x / p);
    const T frac = static_cast<T>(rv - fl_floor(rv));
    if (frac == T(0)) return x;
    T r;
    if (MODE >= ARX_ROUND_HALF_DOWN && frac != T(0.5)) {
      r = round_half_away(rv);
    } else if constexpr (MODE == ARX_ROUND_DOWN || MODE == ARX_ROUND_HALF_DOWN) {
      r = fl_floor(rv);
    } else if constexpr (MODE == ARX_ROUND_UP || MODE == ARX_ROUND_HALF_UP) {
      r = fl_ceil(rv);
    } else if constexpr (MODE == ARX_ROUND_TOWARDS_ZERO || MODE == ARX_ROUND_HALF_TOWARDS_ZERO) {
      r = fl_trunc(rv);
    } else if constexpr (MODE == ARX_ROUND_TOWARDS_INFINITY || MODE == ARX_ROUND_HALF_TOWARDS_INFINITY) {
      r = sign_bit(rv) ? fl_floor(rv) : fl_ceil(rv);
    } else if constexpr (MODE == ARX_ROUND_HALF_TO_EVEN) {
      r = static_cast<T>(round_half_away(static_cast<T>(rv * T(0.5))) * T(2));
    } else {
      const T h = static_cast<T>(rv * T(0.5));
      r = static_cast<T>(fl_floor(h) + fl_ceil(h));
    }
    r = UP ? static_cast<T>(r / p) : static_cast<T>(r * p);
    if (!__builtin_isfinite(r)) {
      *fail = true;
      return x;
    }
    return r;
  }
};

// What the integer rule decides for one value: shared by the kernel and by the host, which words the Status of the
// failing row from it.
struct RoundIntChoice {
  bool exact;   // rem == 0: the value stays
  bool away;    // otherwise: tz +- m (else tz)
  bool tie;     // a half mode met 2 |rem| == m
};
template <typename T>
__host__ __device__ __forceinline__ RoundIntChoice round_int_choice(T v, T m, int mode, T* tz) {
  const T q = static_cast<T>(v / m);
  const T rem = static_cast<T>(v - q * m);
  *tz = static_cast<T>(v - rem);
  RoundIntChoice c{rem == 0, false, false};
  if (c.exact) return c;
  const bool neg = v < T(0);
  switch (mode) {
    case ARX_ROUND_DOWN: c.away = neg; break;
    case ARX_ROUND_UP: c.away = !neg; break;
    case ARX_ROUND_TOWARDS_ZERO: c.away = false; break;
    case ARX_ROUND_TOWARDS_INFINITY: c.away = true; break;
    default: {
      // m <= max(T) / 2 (the entry point refuses a larger one in a half mode): 2 |rem| < 2 m fits 64 bits
      const uint64_t r2 = 2 * (neg ? uint64_t(0) - static_cast<uint64_t>(static_cast<int64_t>(rem)) : static_cast<uint64_t>(rem));
      const uint64_t um = static_cast<uint64_t>(m);
      if (r2 != um) {
        c.away = r2 > um;
      } else {
        c.tie = true;
        const bool odd = (q & T(1)) != 0;
        c.away = mode == ARX_ROUND_HALF_DOWN ? neg : mode == ARX_ROUND_HALF_UP ? !neg : mode == ARX_ROUND_HALF_TOWARDS_ZERO ? false
                 : mode == ARX_ROUND_HALF_TOWARDS_INFINITY ? true : mode == ARX_ROUND_HALF_TO_EVEN ? odd : !odd;
      }
    }
  }
  return c;
}

template <typename T, int MODE>
struct RoundIntOp {
  using Out = T;
  static constexpr bool kCanFail = true;
  T m;
  __device__ __forceinline__ T operator()(T v, bool* fail) const {
    T tz;
    const RoundIntChoice c = round_int_choice<T>(v, m, MODE, &tz);
    if (c.exact) return v;
    if (!c.away) return tz;
    T r;
    const bool overflow = v < T(0) ? __builtin_sub_overflow(tz, m, &r) : __builtin_add_overflow(tz, m, &r);
    if (overflow) {
      *fail = true;
      return v;
    }
    return r;
  }
};

// ---------------------------------------------------------------- the streaming kernel
template <typename T, int N>
struct alignas(sizeof(T) * N >= 16 ? 16 : sizeof(T) * N) UnaryVec {
  T v[N];
};

template <typename T, class Op>
__global__ __launch_bounds__(kBlock) void unary_kernel(const T* __restrict__ in, Bits valid, int64_t n, typename Op::Out* __restrict__ out,
                                                       unsigned long long* __restrict__ errors, Op op) {
  using O = typename Op::Out;
  constexpr int E = 16 / static_cast<int>(sizeof(T));   // rows of a lane's 16 bytes
  const int64_t nchunks = (n + E - 1) / E;
  const int64_t per_block = static_cast<int64_t>(kBlock) * kUnarySteps;
  unsigned long long last_failure = 0;   // (a thread's rows only grow: the last one it sees is its largest)
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * per_block; base < nchunks; base += static_cast<int64_t>(gridDim.x) * per_block) {
    UnaryVec<T, E> v[kUnarySteps];
#pragma unroll
    for (int k = 0; k < kUnarySteps; ++k) {
      const int64_t row0 = (base + k * kBlock + threadIdx.x) * E;
      if (row0 + E <= n) {
        __builtin_memcpy(&v[k], in + row0, 16);
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) v[k].v[e] = row0 + e < n ? in[row0 + e] : T(0);
      }
    }
#pragma unroll
    for (int k = 0; k < kUnarySteps; ++k) {
      const int64_t row0 = (base + k * kBlock + threadIdx.x) * E;
      UnaryVec<O, E> r;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        bool fail = false;
        r.v[e] = op(v[k].v[e], &fail);
        if constexpr (Op::kCanFail) {
          const int64_t row = row0 + e;
          if (fail && row < n && ((load_word(valid, row >> 6) >> (row & 63)) & 1ull) != 0) last_failure = static_cast<unsigned long long>(row) + 1;
        }
      }
      if (row0 + E <= n) {
        __builtin_memcpy(out + row0, &r, sizeof(O) * E);
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          if (row0 + e < n) out[row0 + e] = r.v[e];
        }
      }
    }
  }
  if constexpr (Op::kCanFail) {
    if (last_failure != 0) atomicMax(errors, last_failure);
  }
}

template <typename T, class Op>
static void unary_launch(hipStream_t st, const ArxSpan* values, void* out, uint64_t* errors, Op op) {
  constexpr int E = 16 / static_cast<int>(sizeof(T));
  const int64_t n = values->length;
  const int64_t nchunks = ceil_div(n, E);
  const unsigned grid = static_cast<unsigned>(
      std::max<int64_t>(1, std::min<int64_t>(ceil_div(nchunks, static_cast<int64_t>(kBlock) * kUnarySteps), kUnaryMaxBlocks)));
  hipLaunchKernelGGL((unary_kernel<T, Op>), dim3(grid), dim3(kBlock), 0, st, static_cast<const T*>(values->data) + values->offset,
                     make_bits(values->null_count == 0 ? nullptr : values->validity, values->offset, n), n,
                     static_cast<typename Op::Out*>(out), reinterpret_cast<unsigned long long*>(errors), op);
}

// ---------------------------------------------------------------- host side: types, scales, texts
static const char* const kNumTypeNames[] = {"int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64", "float", "double"};
static const char* const kUnaryNames[] = {"negate", "abs", "sign", "floor", "ceil", "trunc"};
static bool num_type_ok(int t) { return t >= ARX_NUM_INT8 && t <= ARX_NUM_FLOAT64; }
static bool num_type_float(int t) { return t == ARX_NUM_FLOAT32 || t == ARX_NUM_FLOAT64; }
static bool num_type_unsigned(int t) { return t <= ARX_NUM_UINT64 && (t & 1) != 0; }

// pow10 of the reference: a table of FLOAT literals up to 10^15 — also for double, whose pow10(11) is 99999997952 —
// then one multiplication by ten per further step.
template <typename T>
static T round_pow10(int64_t p) {
  static const float kLut[] = {1e0f, 1e1f, 1e2f, 1e3f, 1e4f, 1e5f, 1e6f, 1e7f, 1e8f, 1e9f, 1e10f, 1e11f, 1e12f, 1e13f, 1e14f, 1e15f};
  volatile T r = static_cast<T>(kLut[std::min<int64_t>(p, 15)]);   // (volatile: each product rounded to T, on any host)
  for (int64_t i = 16; i <= p && std::isfinite(static_cast<T>(r)); ++i) r = static_cast<T>(r * T(10));
  return r;
}

// the arguments of a rounding call, checked and reduced to what the kernel takes
struct RoundPlan {
  bool is_float = false;
  bool up = false;          // floats: scale up first (ndigits > 0)
  double scale_f64 = 1.0;   // floats: p
  float scale_f32 = 1.0f;
  uint64_t m = 1;           // integers: the multiple, positive (its bits for the signed types too)
};

template <typename T>
static int round_plan_int(int kind, int mode, int num_type, int64_t ndigits, const void* multiple, RoundPlan* plan) {
  const uint64_t max = static_cast<uint64_t>(std::numeric_limits<T>::max());
  if (kind == ARX_ROUND_DIGITS) {
    if (ndigits >= 0) {
      plan->m = 1;   // (every value is its own multiple of one: the input comes back)
      return ARX_OK;
    }
    uint64_t m = 1;
    bool fits = ndigits >= -19;
    for (int64_t i = 0; fits && i < -ndigits; ++i) {
      fits = m <= max / 10;
      m *= 10;
    }
    if (!fits) {
      set_error("Rounding to %lld digits is out of range for type %s", static_cast<long long>(ndigits), kNumTypeNames[num_type]);
      return ARX_INVALID;
    }
    plan->m = m;
  } else {
    const T m = *static_cast<const T*>(multiple);
    if (m <= 0) {
      set_error("Rounding multiple must be positive");
      return ARX_INVALID;
    }
    plan->m = static_cast<uint64_t>(m);
  }
  if (mode >= ARX_ROUND_HALF_DOWN && plan->m > max / 2) {
    // the reference's 2 |rem| wraps there, and its results with it: not reproduced on the device
    set_error("arrow_amd: %s of %s to the multiple %llu in a half_* round mode on device-resident arrays: a multiple above half the "
              "type's maximum (%llu) has no device kernel", kind == ARX_ROUND_DIGITS ? "round" : "round_to_multiple", kNumTypeNames[num_type],
              static_cast<unsigned long long>(plan->m), static_cast<unsigned long long>(max / 2));
    return ARX_NOT_IMPLEMENTED;
  }
  return ARX_OK;
}

static int round_plan(const char* who, int kind, int mode, int num_type, int64_t ndigits, const void* multiple, RoundPlan* plan) {
  if ((kind != ARX_ROUND_DIGITS && kind != ARX_ROUND_MULTIPLE) || mode < ARX_ROUND_DOWN || mode > ARX_ROUND_HALF_TO_ODD || !num_type_ok(num_type)) {
    set_error("%s: no kernel for kind %d, round mode %d, numeric type %d", who, kind, mode, num_type);
    return ARX_INVALID;
  }
  if (kind == ARX_ROUND_MULTIPLE && multiple == nullptr) {
    set_error("%s: NULL multiple", who);
    return ARX_INVALID;
  }
  plan->is_float = num_type_float(num_type);
  if (plan->is_float) {
    if (kind == ARX_ROUND_DIGITS) {
      const int64_t p = ndigits < 0 ? (ndigits == INT64_MIN ? INT64_MAX : -ndigits) : ndigits;
      plan->up = ndigits > 0;
      plan->scale_f64 = round_pow10<double>(p);
      plan->scale_f32 = round_pow10<float>(p);
    } else {
      plan->scale_f64 = num_type == ARX_NUM_FLOAT64 ? *static_cast<const double*>(multiple) : 1.0;
      plan->scale_f32 = num_type == ARX_NUM_FLOAT32 ? *static_cast<const float*>(multiple) : 1.0f;
      if (!(plan->scale_f64 > 0.0) || !(plan->scale_f32 > 0.0f)) {
        set_error("Rounding multiple must be positive");
        return ARX_INVALID;
      }
    }
    return ARX_OK;
  }
  switch (num_type) {
    case ARX_NUM_INT8: return round_plan_int<int8_t>(kind, mode, num_type, ndigits, multiple, plan);
    case ARX_NUM_UINT8: return round_plan_int<uint8_t>(kind, mode, num_type, ndigits, multiple, plan);
    case ARX_NUM_INT16: return round_plan_int<int16_t>(kind, mode, num_type, ndigits, multiple, plan);
    case ARX_NUM_UINT16: return round_plan_int<uint16_t>(kind, mode, num_type, ndigits, multiple, plan);
    case ARX_NUM_INT32: return round_plan_int<int32_t>(kind, mode, num_type, ndigits, multiple, plan);
    case ARX_NUM_UINT32: return round_plan_int<uint32_t>(kind, mode, num_type, ndigits, multiple, plan);
    case ARX_NUM_INT64: return round_plan_int<int64_t>(kind, mode, num_type, ndigits, multiple, plan);
    default: return round_plan_int<uint64_t>(kind, mode, num_type, ndigits, multiple, plan);
  }
}

static int unary_span_ok(const char* who, const ArxSpan* values, const void* out, bool needs_errors, const uint64_t* errors) {
  if (values == nullptr) {
    set_error("%s: NULL values", who);
    return ARX_INVALID;
  }
  if (values->length < 0 || values->offset < 0) {
    set_error("%s: negative %s", who, values->length < 0 ? "length" : "offset");
    return ARX_INVALID;
  }
  if (values->length > 0 && (values->data == nullptr || out == nullptr)) {
    set_error("%s: NULL %s", who, out == nullptr ? "out" : "data buffer of values");
    return ARX_INVALID;
  }
  if (values->length > 0 && needs_errors && errors == nullptr) {
    set_error("%s: NULL errors, but a row of this call can fail", who);
    return ARX_INVALID;
  }
  return ARX_OK;
}

template <typename T, int MODE>
static void round_launch_mode(hipStream_t st, const RoundPlan& plan, const ArxSpan* values, void* out, uint64_t* errors) {
  if constexpr (std::is_floating_point<T>::value) {
    const T p = std::is_same<T, float>::value ? static_cast<T>(plan.scale_f32) : static_cast<T>(plan.scale_f64);
    if (plan.up) unary_launch<T>(st, values, out, errors, RoundFloatOp<T, MODE, true>{p});
    else unary_launch<T>(st, values, out, errors, RoundFloatOp<T, MODE, false>{p});
  } else {
    unary_launch<T>(st, values, out, errors, RoundIntOp<T, MODE>{static_cast<T>(plan.m)});
  }
}

template <typename T>
static void round_launch(int mode, hipStream_t st, const RoundPlan& plan, const ArxSpan* values, void* out, uint64_t* errors) {
  switch (mode) {
#define ARX_ROUND_MODE(M) case M: round_launch_mode<T, M>(st, plan, values, out, errors); break;
    ARX_ROUND_MODE(ARX_ROUND_DOWN) ARX_ROUND_MODE(ARX_ROUND_UP) ARX_ROUND_MODE(ARX_ROUND_TOWARDS_ZERO)
    ARX_ROUND_MODE(ARX_ROUND_TOWARDS_INFINITY) ARX_ROUND_MODE(ARX_ROUND_HALF_DOWN) ARX_ROUND_MODE(ARX_ROUND_HALF_UP)
    ARX_ROUND_MODE(ARX_ROUND_HALF_TOWARDS_ZERO) ARX_ROUND_MODE(ARX_ROUND_HALF_TOWARDS_INFINITY)
    ARX_ROUND_MODE(ARX_ROUND_HALF_TO_EVEN) ARX_ROUND_MODE(ARX_ROUND_HALF_TO_ODD)
#undef ARX_ROUND_MODE
  }
}

// "Rounding <v> up|down to multiple(s) of <m> would overflow" for the integer v that failed
template <typename T>
static void round_int_error_text(T v, uint64_t m, int mode) {
  T tz;
  const RoundIntChoice c = round_int_choice<T>(v, static_cast<T>(m), mode, &tz);
  const bool plural = mode >= ARX_ROUND_HALF_DOWN && !c.tie;
  if (std::is_signed<T>::value) {
    set_error("Rounding %lld %s to multiple%s of %llu would overflow", static_cast<long long>(v), v < T(0) ? "down" : "up", plural ? "s" : "",
              static_cast<unsigned long long>(m));
  } else {
    set_error("Rounding %llu up to multiple%s of %llu would overflow", static_cast<unsigned long long>(v), plural ? "s" : "",
              static_cast<unsigned long long>(m));
  }
}

#define ARX_UNARY_ALL_TYPES(CASE)                                                                                      \
  CASE(ARX_NUM_INT8, int8_t) CASE(ARX_NUM_UINT8, uint8_t) CASE(ARX_NUM_INT16, int16_t) CASE(ARX_NUM_UINT16, uint16_t) \
  CASE(ARX_NUM_INT32, int32_t) CASE(ARX_NUM_UINT32, uint32_t) CASE(ARX_NUM_INT64, int64_t) CASE(ARX_NUM_UINT64, uint64_t) \
  CASE(ARX_NUM_FLOAT32, float) CASE(ARX_NUM_FLOAT64, double)

extern "C" {

int arx_unary_numeric(int op, int checked, int num_type, const ArxSpan* values, void* out, uint64_t* errors, void* stream) {
  const bool known = op >= ARX_UNARY_NEGATE && op <= ARX_UNARY_TRUNC && num_type_ok(num_type);
  const bool has_checked = op == ARX_UNARY_NEGATE || op == ARX_UNARY_ABS;
  if (!known || (checked != 0 && !has_checked) || (op >= ARX_UNARY_FLOOR && !num_type_float(num_type)) ||
      (op == ARX_UNARY_NEGATE && checked != 0 && num_type_unsigned(num_type))) {
    set_error("arx_unary_numeric: no kernel for op %d (%s%s) of numeric type %d", op, known ? kUnaryNames[op] : "?",
              checked != 0 ? "_checked" : "", num_type);
    return ARX_INVALID;
  }
  const bool can_fail = checked != 0 && !num_type_float(num_type) && !num_type_unsigned(num_type);
  const int rc = unary_span_ok("arx_unary_numeric", values, out, can_fail, errors);
  if (rc != ARX_OK) return rc;
  if (values->length == 0) return ARX_OK;
  hipStream_t st = as_stream(stream);
#define ARX_UNARY_NEGATE_CASE(CODE, T)                                                                 \
  case CODE:                                                                                           \
    if (can_fail) unary_launch<T>(st, values, out, errors, NegateOp<T, true>{});                       \
    else unary_launch<T>(st, values, out, errors, NegateOp<T, false>{});                               \
    break;
#define ARX_UNARY_ABS_CASE(CODE, T)                                                                    \
  case CODE:                                                                                           \
    if (can_fail) unary_launch<T>(st, values, out, errors, AbsOp<T, true>{});                          \
    else unary_launch<T>(st, values, out, errors, AbsOp<T, false>{});                                  \
    break;
#define ARX_UNARY_SIGN_CASE(CODE, T) \
  case CODE: unary_launch<T>(st, values, out, errors, SignOp<T>{}); break;
  switch (op) {
    case ARX_UNARY_NEGATE:
      switch (num_type) { ARX_UNARY_ALL_TYPES(ARX_UNARY_NEGATE_CASE) }
      break;
    case ARX_UNARY_ABS:
      switch (num_type) { ARX_UNARY_ALL_TYPES(ARX_UNARY_ABS_CASE) }
      break;
    case ARX_UNARY_SIGN:
      switch (num_type) { ARX_UNARY_ALL_TYPES(ARX_UNARY_SIGN_CASE) }
      break;
    case ARX_UNARY_FLOOR:
      if (num_type == ARX_NUM_FLOAT32) unary_launch<float>(st, values, out, errors, FloorOp<float, ARX_UNARY_FLOOR>{});
      else unary_launch<double>(st, values, out, errors, FloorOp<double, ARX_UNARY_FLOOR>{});
      break;
    case ARX_UNARY_CEIL:
      if (num_type == ARX_NUM_FLOAT32) unary_launch<float>(st, values, out, errors, FloorOp<float, ARX_UNARY_CEIL>{});
      else unary_launch<double>(st, values, out, errors, FloorOp<double, ARX_UNARY_CEIL>{});
      break;
    default:
      if (num_type == ARX_NUM_FLOAT32) unary_launch<float>(st, values, out, errors, FloorOp<float, ARX_UNARY_TRUNC>{});
      else unary_launch<double>(st, values, out, errors, FloorOp<double, ARX_UNARY_TRUNC>{});
      break;
  }
#undef ARX_UNARY_NEGATE_CASE
#undef ARX_UNARY_ABS_CASE
#undef ARX_UNARY_SIGN_CASE
  ARX_CHECK_LAUNCH("unary_kernel");
  g_unary_arith_launches.fetch_add(1, std::memory_order_relaxed);
  return ARX_OK;
}

int arx_round_numeric(int kind, int mode, int num_type, const ArxSpan* values, int64_t ndigits, const void* multiple, void* out,
                      uint64_t* errors, void* stream) {
  RoundPlan plan;
  int rc = round_plan("arx_round_numeric", kind, mode, num_type, ndigits, multiple, &plan);
  if (rc != ARX_OK) return rc;
  rc = unary_span_ok("arx_round_numeric", values, out, true, errors);
  if (rc != ARX_OK) return rc;
  if (values->length == 0) return ARX_OK;
  hipStream_t st = as_stream(stream);
  switch (num_type) {
#define ARX_ROUND_CASE(CODE, T) \
  case CODE: round_launch<T>(mode, st, plan, values, out, errors); break;
    ARX_UNARY_ALL_TYPES(ARX_ROUND_CASE)
#undef ARX_ROUND_CASE
  }
  ARX_CHECK_LAUNCH("unary_kernel (round)");
  g_round_launches.fetch_add(1, std::memory_order_relaxed);
  return ARX_OK;
}

int arx_round_status(int kind, int mode, int num_type, const ArxSpan* values, int64_t ndigits, const void* multiple, const uint64_t* errors,
                     void* stream) {
  RoundPlan plan;
  int rc = round_plan("arx_round_status", kind, mode, num_type, ndigits, multiple, &plan);
  if (rc != ARX_OK) return rc;
  rc = unary_span_ok("arx_round_status", values, values != nullptr ? values->data : nullptr, true, errors);
  if (rc != ARX_OK) return rc;
  hipStream_t st = as_stream(stream);
  if (values->length == 0) {
    ARX_HIP(hipStreamSynchronize(st));
    return ARX_OK;
  }
  uint64_t last = 0;
  ARX_HIP(hipMemcpyAsync(&last, errors, sizeof(last), hipMemcpyDeviceToHost, st));
  ARX_HIP(hipStreamSynchronize(st));
  if (last == 0) return ARX_OK;
  if (last > static_cast<uint64_t>(values->length)) {
    set_error("arx_round_status: the error word names row %llu of %lld", static_cast<unsigned long long>(last - 1),
              static_cast<long long>(values->length));
    return ARX_INVALID;
  }
  if (plan.is_float) {
    set_error("overflow occurred during rounding");
    return ARX_INVALID;
  }
  const int width = 1 << (num_type >> 1);
  uint64_t raw = 0;
  ARX_HIP(hipMemcpyAsync(&raw, static_cast<const char*>(values->data) + (values->offset + static_cast<int64_t>(last - 1)) * width, width,
                         hipMemcpyDeviceToHost, st));
  ARX_HIP(hipStreamSynchronize(st));
  switch (num_type) {
#define ARX_ROUND_TEXT(CODE, T) \
  case CODE: { T v; memcpy(&v, &raw, sizeof(T)); round_int_error_text<T>(v, plan.m, mode); break; }
    ARX_ROUND_TEXT(ARX_NUM_INT8, int8_t) ARX_ROUND_TEXT(ARX_NUM_UINT8, uint8_t) ARX_ROUND_TEXT(ARX_NUM_INT16, int16_t)
    ARX_ROUND_TEXT(ARX_NUM_UINT16, uint16_t) ARX_ROUND_TEXT(ARX_NUM_INT32, int32_t) ARX_ROUND_TEXT(ARX_NUM_UINT32, uint32_t)
    ARX_ROUND_TEXT(ARX_NUM_INT64, int64_t) ARX_ROUND_TEXT(ARX_NUM_UINT64, uint64_t)
#undef ARX_ROUND_TEXT
  }
  return ARX_INVALID;
}

}  // extern "C"

#undef ARX_UNARY_ALL_TYPES

}  // namespace arx

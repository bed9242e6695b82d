// if_else(cond, left, right) for one fixed-width (or boolean) type on gfx950 — what CASE WHEN .. THEN .. ELSE .. END and
// every "clip / replace / flag" projection lowers to.
//
// What it restates (semantics only):
//   IfElseFunctor / RunIfElseLoop   cpp/src/arrow/compute/kernels/scalar_if_else.cc   (fixed-width types, boolean)
// out[i] = cond[i] ? left[i] : right[i]; null where cond is null (whatever its data bit says), else the validity of the
// chosen operand.  On the 64-row words of the bitmaps: take_l = c & cv, take_r = ~c & cv,
// valid = (take_l & lv) | (take_r & rv).  A null result slot is written as zero (as coalesce2_kernel does), so two
// builds' outputs compare byte for byte.  left / right: an array, a valid scalar or a null scalar each.
//
// Shape, widths 8 and 16: a wave takes kIfElseWords consecutive words (256 rows), lane = row within a word (widths 1, 2
// and 4: if_else_packed_kernel below, the same with 8 / W rows a lane).  The bitmap words are
// wave-uniform (scalar loads); all value loads of the wave's words are issued before the first select, so a lane has up
// to 2 x kIfElseWords loads in flight; lane 0 stores the validity words.  A side none of a word's 64 rows takes (or takes
// only as null) is not loaded: the branch is wave-uniform, and a clustered condition (a sorted or partitioned column)
// then reads one value stream instead of two.  -DARX_IF_ELSE_SKIP=0 compiles the plain form (both sides always loaded):
// the A/B of DESIGN.md 4.19.
// Booleans: 64 rows per lane with bit operations.  HBM: both value streams and 3 to 5 bits a row in, the result out.
#include "arx_common.h"

#include <algorithm>

#ifndef ARX_IF_ELSE_SKIP
#define ARX_IF_ELSE_SKIP 1
#endif

namespace arx {

// rows one wave takes at a time (tests/test_if_else.py: ROWS_PER_WAVE): 64 x kIfElseWords at widths 8 and 16,
// 64 x (8 / W) x kIfElsePackedSteps at widths 1, 2 and 4
constexpr int kIfElseWords = 4;
constexpr int kIfElsePackedSteps = 2;
constexpr int64_t kIfElseMaxBlocks = 1 << 20;   // workgroups of a launch (a wave strides over what is left: past 2^30 rows)

static std::atomic<int64_t> g_if_else_launches{0};          // if_else_kernel<T>: widths 8 and 16
static std::atomic<int64_t> g_if_else_packed_launches{0};   // if_else_packed_kernel<T>: widths 1, 2 and 4
static std::atomic<int64_t> g_if_else_bool_launches{0};     // if_else_bool_kernel
static constexpr CounterRow kIfElseCounters[] = {
    {"if_else_launches", &g_if_else_launches},
    {"if_else_packed_launches", &g_if_else_packed_launches},
    {"if_else_bool_launches", &g_if_else_bool_launches},
};
CounterTable if_else_counters() { return counter_table(kIfElseCounters); }

struct U128 {
  uint64_t lo, hi;
};

enum { kOperandArray = 0, kOperandScalar = 1, kOperandNull = 2 };

// left / right of a fixed-width call: `data` is logical element 0 (arrays), `valid` the array's bitmap (NULL base: none)
template <typename T>
struct IfElseOperand {
  const T* data;
  T scalar;
  Bits valid;
  int kind;
};

// validity word w of an operand: the bitmap's, all ones (below `length`) for a valid scalar, zero for a null scalar
__device__ __forceinline__ uint64_t operand_valid_word(const Bits& valid, int kind, int64_t w) {
  return kind == kOperandNull ? 0ull : load_word(valid, w);
}

template <typename T, bool kSkip>
__global__ __launch_bounds__(kBlock) void if_else_kernel(Bits c, Bits cv, IfElseOperand<T> l, IfElseOperand<T> r, int64_t n,
                                                         T* __restrict__ out, uint64_t* __restrict__ out_valid) {
  const int lane = lane_id();
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  const int64_t nwords = (n + 63) >> 6;
  const int64_t nsteps = (nwords + kIfElseWords - 1) / kIfElseWords;
  for (int64_t s = wave; s < nsteps; s += nwaves) {
    const int64_t w0 = s * kIfElseWords;
    uint64_t need_l[kIfElseWords], need_r[kIfElseWords];
    T lv[kIfElseWords], rv[kIfElseWords];
#pragma unroll
    for (int k = 0; k < kIfElseWords; ++k) {
      const int64_t w = w0 + k;   // (a word past the last one reads as zero everywhere: nothing is loaded or stored for it)
      const uint64_t cvw = load_word(cv, w);
      const uint64_t take_l = load_word(c, w) & cvw;
      need_l[k] = take_l & operand_valid_word(l.valid, l.kind, w);
      need_r[k] = (cvw & ~take_l) & operand_valid_word(r.valid, r.kind, w);
      const int64_t i = (w << 6) + lane;
      lv[k] = l.scalar;
      rv[k] = r.scalar;
      const bool want_l = !kSkip || need_l[k] != 0, want_r = !kSkip || need_r[k] != 0;   // (wave-uniform)
      if (l.kind == kOperandArray && want_l && i < n) lv[k] = l.data[i];
      if (r.kind == kOperandArray && want_r && i < n) rv[k] = r.data[i];
    }
#pragma unroll
    for (int k = 0; k < kIfElseWords; ++k) {
      const int64_t w = w0 + k;
      const int64_t i = (w << 6) + lane;
      if (i < n) out[i] = ((need_l[k] >> lane) & 1ull) ? lv[k] : (((need_r[k] >> lane) & 1ull) ? rv[k] : T{});
      if (lane == 0 && out_valid != nullptr && w < nwords) out_valid[w] = need_l[k] | need_r[k];
    }
  }
}

// widths 1, 2 and 4: a lane takes kV = 8 / W consecutive rows, so that every load and store moves 8 bytes a lane (one
// wave instruction covers kV words) instead of 1, 2 or 4; kIfElsePackedSteps such loads of each side are in flight.  The
// rows of a lane lie in one word: word lane / (64 / kV) of the step's kV, from bit (lane % (64 / kV)) * kV.  The inputs
// carry their own element offsets, so their 8 bytes are read at any alignment (global memory takes it); a lane whose rows
// straddle `n` reads and writes them one by one.
template <typename T, bool kSkip>
__global__ __launch_bounds__(kBlock) void if_else_packed_kernel(Bits c, Bits cv, IfElseOperand<T> l, IfElseOperand<T> r, int64_t n,
                                                                T* __restrict__ out, uint64_t* __restrict__ out_valid) {
  constexpr int kV = 8 / static_cast<int>(sizeof(T));
  constexpr int kLanesPerWord = 64 / kV;
  constexpr int kBits = 8 * static_cast<int>(sizeof(T));
  constexpr uint64_t kElement = (uint64_t(1) << kBits) - 1;
  const int lane = lane_id();
  const int my_word = lane / kLanesPerWord;
  const int my_shift = (lane % kLanesPerWord) * kV;
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  const int64_t nwords = (n + 63) >> 6;
  const int64_t nsteps = (nwords + kV * kIfElsePackedSteps - 1) / (kV * kIfElsePackedSteps);
  uint64_t l_scalar = 0, r_scalar = 0;   // the scalars, kV times over
#pragma unroll
  for (int j = 0; j < kV; ++j) {
    l_scalar |= static_cast<uint64_t>(l.scalar) << (j * kBits);
    r_scalar |= static_cast<uint64_t>(r.scalar) << (j * kBits);
  }
  for (int64_t s = wave; s < nsteps; s += nwaves) {
    uint64_t valid_l[kIfElsePackedSteps], valid_r[kIfElsePackedSteps];   // this lane's word of the step
    uint64_t lv[kIfElsePackedSteps], rv[kIfElsePackedSteps];
#pragma unroll
    for (int k = 0; k < kIfElsePackedSteps; ++k) {
      const int64_t w0 = (s * kIfElsePackedSteps + k) * kV;
      uint64_t any_l = 0, any_r = 0;
      valid_l[k] = valid_r[k] = 0;
#pragma unroll
      for (int j = 0; j < kV; ++j) {
        const int64_t w = w0 + j;
        const uint64_t cvw = load_word(cv, w);
        const uint64_t take_l = load_word(c, w) & cvw;
        const uint64_t need_l = take_l & operand_valid_word(l.valid, l.kind, w);
        const uint64_t need_r = (cvw & ~take_l) & operand_valid_word(r.valid, r.kind, w);
        any_l |= need_l;
        any_r |= need_r;
        if (my_word == j) {
          valid_l[k] = need_l;
          valid_r[k] = need_r;
        }
      }
      const int64_t row0 = (w0 << 6) + lane * kV;
      lv[k] = l_scalar;
      rv[k] = r_scalar;
      const bool want_l = !kSkip || any_l != 0, want_r = !kSkip || any_r != 0;   // (wave-uniform)
      if (l.kind == kOperandArray && want_l) {
        if (row0 + kV <= n) {
          __builtin_memcpy(&lv[k], l.data + row0, 8);
        } else {
          lv[k] = 0;
          for (int j = 0; j < kV; ++j) {
            if (row0 + j < n) lv[k] |= static_cast<uint64_t>(l.data[row0 + j]) << (j * kBits);
          }
        }
      }
      if (r.kind == kOperandArray && want_r) {
        if (row0 + kV <= n) {
          __builtin_memcpy(&rv[k], r.data + row0, 8);
        } else {
          rv[k] = 0;
          for (int j = 0; j < kV; ++j) {
            if (row0 + j < n) rv[k] |= static_cast<uint64_t>(r.data[row0 + j]) << (j * kBits);
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kIfElsePackedSteps; ++k) {
      const int64_t w0 = (s * kIfElsePackedSteps + k) * kV;
      const int64_t row0 = (w0 << 6) + lane * kV;
      uint64_t mask_l = 0, mask_r = 0;
#pragma unroll
      for (int j = 0; j < kV; ++j) {
        if ((valid_l[k] >> (my_shift + j)) & 1ull) mask_l |= kElement << (j * kBits);
        if ((valid_r[k] >> (my_shift + j)) & 1ull) mask_r |= kElement << (j * kBits);
      }
      const uint64_t v = (lv[k] & mask_l) | (rv[k] & mask_r);   // (a null result slot: zero)
      if (row0 + kV <= n) {
        __builtin_memcpy(out + row0, &v, 8);
      } else {
        for (int j = 0; j < kV; ++j) {
          if (row0 + j < n) out[row0 + j] = static_cast<T>(v >> (j * kBits));
        }
      }
      if (lane % kLanesPerWord == 0 && out_valid != nullptr && w0 + my_word < nwords) out_valid[w0 + my_word] = valid_l[k] | valid_r[k];
    }
  }
}

// booleans: 64 rows per lane
__global__ __launch_bounds__(kBlock) void if_else_bool_kernel(Bits c, Bits cv, Bits l, Bits lvalid, int l_kind, int l_scalar, Bits r,
                                                              Bits rvalid, int r_kind, int r_scalar, int64_t n,
                                                              uint64_t* __restrict__ out, uint64_t* __restrict__ out_valid) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  const int64_t nwords = (n + 63) >> 6;
  for (int64_t w = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; w < nwords; w += stride) {
    const uint64_t cvw = load_word(cv, w);
    const uint64_t take_l = load_word(c, w) & cvw;
    const uint64_t need_l = take_l & operand_valid_word(lvalid, l_kind, w);
    const uint64_t need_r = (cvw & ~take_l) & operand_valid_word(rvalid, r_kind, w);
    const uint64_t dl = l_kind == kOperandArray ? load_word(l, w) : (l_scalar ? ~0ull : 0ull);
    const uint64_t dr = r_kind == kOperandArray ? load_word(r, w) : (r_scalar ? ~0ull : 0ull);
    out[w] = (need_l & dl) | (need_r & dr);
    if (out_valid != nullptr) out_valid[w] = need_l | need_r;
  }
}

static int operand_kind(const ArxSpan* span, const void* scalar) {
  return span != nullptr ? kOperandArray : (scalar != nullptr ? kOperandScalar : kOperandNull);
}
static bool has_bitmap(const ArxSpan* span) { return span != nullptr && span->validity != nullptr && span->null_count != 0; }
static Bits operand_valid_bits(const ArxSpan* span, int64_t length) {
  return make_bits(has_bitmap(span) ? span->validity : nullptr, span != nullptr ? span->offset : 0, length);
}

template <typename T>
static IfElseOperand<T> make_operand(const ArxSpan* span, const void* scalar, int64_t length) {
  IfElseOperand<T> o;
  o.data = span != nullptr ? static_cast<const T*>(span->data) + span->offset : nullptr;
  o.scalar = T{};
  if (span == nullptr && scalar != nullptr) __builtin_memcpy(&o.scalar, scalar, sizeof(T));
  o.valid = operand_valid_bits(span, length);
  o.kind = operand_kind(span, scalar);
  return o;
}

extern "C" {

int arx_if_else(int byte_width, const ArxSpan* cond, const ArxSpan* left, const void* left_scalar, const ArxSpan* right,
                const void* right_scalar, int64_t length, void* out_data, void* out_validity, void* stream) {
  if (byte_width != 0 && byte_width != 1 && byte_width != 2 && byte_width != 4 && byte_width != 8 && byte_width != 16) {
    set_error("arx_if_else: byte_width %d (0 = boolean, 1, 2, 4, 8, 16)", byte_width);
    return ARX_INVALID;
  }
  if (length < 0) {
    set_error("arx_if_else: negative length %lld", static_cast<long long>(length));
    return ARX_INVALID;
  }
  if (cond == nullptr) {
    set_error("arx_if_else: NULL cond");
    return ARX_INVALID;
  }
  const struct { const char* name; const ArxSpan* span; const void* scalar; } operands[] = {
      {"cond", cond, nullptr}, {"left", left, left_scalar}, {"right", right, right_scalar}};
  for (const auto& o : operands) {
    if (o.span != nullptr && o.span->length != length) {
      set_error("arx_if_else: span length %lld of %s is not length %lld", static_cast<long long>(o.span->length), o.name,
                static_cast<long long>(length));
      return ARX_INVALID;
    }
    if (o.span != nullptr && o.scalar != nullptr) {
      set_error("arx_if_else: %s is given as an array and as a scalar", o.name);
      return ARX_INVALID;
    }
  }
  if (length == 0) return ARX_OK;
  if (out_data == nullptr) {
    set_error("arx_if_else: NULL out_data");
    return ARX_INVALID;
  }
  for (const auto& o : operands) {
    if (o.span != nullptr && o.span->data == nullptr) {
      set_error("arx_if_else: NULL data buffer of %s", o.name);
      return ARX_INVALID;
    }
  }
  const int l_kind = operand_kind(left, left_scalar), r_kind = operand_kind(right, right_scalar);
  const bool may_have_nulls = has_bitmap(cond) || has_bitmap(left) || has_bitmap(right) || l_kind == kOperandNull || r_kind == kOperandNull;
  if (out_validity == nullptr && may_have_nulls) {
    set_error("arx_if_else: NULL out_validity, but an operand has a validity bitmap or is a null scalar");
    return ARX_INVALID;
  }
  const Bits c = make_bits(cond->data, cond->offset, length);
  const Bits cv = operand_valid_bits(cond, length);
  hipStream_t st = as_stream(stream);
  const int64_t nwords = ceil_div(length, 64);
  if (byte_width == 0) {
    const Bits l = left != nullptr ? make_bits(left->data, left->offset, length) : Bits{nullptr, 0, length, 0};
    const Bits r = right != nullptr ? make_bits(right->data, right->offset, length) : Bits{nullptr, 0, length, 0};
    const int ls = left_scalar != nullptr ? (*static_cast<const uint8_t*>(left_scalar) != 0) : 0;
    const int rs = right_scalar != nullptr ? (*static_cast<const uint8_t*>(right_scalar) != 0) : 0;
    const unsigned grid = static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(ceil_div(nwords, kBlock), 1 << 16)));
    hipLaunchKernelGGL(if_else_bool_kernel, dim3(grid), dim3(kBlock), 0, st, c, cv, l, operand_valid_bits(left, length), l_kind, ls, r,
                       operand_valid_bits(right, length), r_kind, rs, length, static_cast<uint64_t*>(out_data),
                       static_cast<uint64_t*>(out_validity));
    ARX_CHECK_LAUNCH("if_else_bool_kernel");
    g_if_else_bool_launches.fetch_add(1, std::memory_order_relaxed);
    return ARX_OK;
  }
  const bool packed = byte_width < 8;
  const int64_t nsteps = ceil_div(nwords, packed ? (8 / byte_width) * kIfElsePackedSteps : kIfElseWords);
  const unsigned grid = static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(ceil_div(nsteps, kWavesPerBlock), kIfElseMaxBlocks)));
#define ARX_IF_ELSE_CASE(W, KERNEL, T)                                                                                       \
  case W:                                                                                                                    \
    hipLaunchKernelGGL((KERNEL<T, ARX_IF_ELSE_SKIP != 0>), dim3(grid), dim3(kBlock), 0, st, c, cv,                            \
                       make_operand<T>(left, left_scalar, length), make_operand<T>(right, right_scalar, length), length,     \
                       static_cast<T*>(out_data), static_cast<uint64_t*>(out_validity));                                     \
    break;
  switch (byte_width) {
    ARX_IF_ELSE_CASE(1, if_else_packed_kernel, uint8_t)
    ARX_IF_ELSE_CASE(2, if_else_packed_kernel, uint16_t)
    ARX_IF_ELSE_CASE(4, if_else_packed_kernel, uint32_t)
    ARX_IF_ELSE_CASE(8, if_else_kernel, uint64_t)
    ARX_IF_ELSE_CASE(16, if_else_kernel, U128)
  }
#undef ARX_IF_ELSE_CASE
  ARX_CHECK_LAUNCH(packed ? "if_else_packed_kernel" : "if_else_kernel");
  (packed ? g_if_else_packed_launches : g_if_else_launches).fetch_add(1, std::memory_order_relaxed);
  return ARX_OK;
}

}  // extern "C"

}  // namespace arx

// The six comparisons of utf8 / binary columns and their large forms: equal, not_equal, greater, greater_equal, less,
// less_equal (CompareKernel on BaseBinaryType, compute/kernels/scalar_compare.cc).  The order is std::string_view's:
// bytes compare as unsigned bytes over the common length, then the shorter row is less.  No UTF-8 awareness, a '\0' is
// an ordinary byte.  The output is a bitmap at offset 0 (bit i = the answer of row i, 0 where either side is null); the
// validity of the result is the intersection of the inputs' and is the caller's (arx_bitmap_copy / arx_bitmap_and).
//
// Operands: array x array, or array x literal.  literal x array is array x literal under the mirrored op
// (a < b  <=>  b > a), so the kernels know two shapes only.  The literal is a device pointer, staged per workgroup in LDS
// up to kPatternLdsCap bytes and read where it lies beyond (string_rows.h).
//
// Two kernels, both ending in one __ballot word for 64 row pairs, written whole by lane 0.
//   rows   one lane per row pair.  equal / not_equal of rows of different length are decided from the offsets: no data
//          byte is read.  Otherwise the lane walks the common length in 8-byte pieces, each side through its own
//          two-word sliding window (Stream8), and stops at the first piece that differs; the order of that piece is the
//          order of its two words byte-swapped, as unsigned integers.
//   waves  one wave per row pair, 64 consecutive pairs a step, one after the other.  Lane j takes the j-th aligned
//          16-byte granule of the LEFT row; the right row's bytes at the same row positions start `d` bytes into ITS
//          j-th aligned granule and end in the (j + 1)-th, which is the next lane's (__shfl_down; lane 63 loads it), so
//          the 16 bytes come out of a funnel shift of two granules.  __ballot / __ffsll find the first granule that
//          differs; no later step runs.
//
// Granule rule: a load touches only an aligned 8- or 16-byte piece that holds at least one byte of the common length
// of a pair of valid rows (of the literal for literal reads).  A null row on either side is not read at all.
#include "string_rows.h"

namespace arx {

namespace {

// auto (path 0): the waves form when a row pair may have to read this many bytes on average: data_bytes_hint / length
// for two arrays (the hint is the sum of both data buffers), twice min(data_bytes_hint / length, literal_length) for an
// array and a literal (no walk goes past the literal's end).  Measured on the MI355X (scripts/exp_string_compare.py,
// profiles/string_compare.txt: `less` of two columns of 2^28 data bytes whose rows are equal but for the last byte): the
// rows form is ahead at 64 bytes a row, 128 a pair (0.545 ms against 1.711 ms), the waves form from 128 bytes a row on
// (0.913 ms against 1.061 ms; 0.469 ms against 1.129 ms at 256, 0.151 ms against 1.278 ms at 1024).  Rows that differ
// in their first bytes favour the rows form at any size, since a lane stops at the first difference while a wave
// still spends a step a pair; the threshold bounds the other case, long shared prefixes.
constexpr int64_t kWavesPathMeanPair = 512;

std::atomic<int64_t> g_compare_row_launches{0}, g_compare_wave_launches{0};

// the answer of `op` for a three-way result c (< 0, 0, > 0)
__device__ __forceinline__ bool answer(int op, int c) {
  switch (op) {
    case ARX_CMP_EQUAL: return c == 0;
    case ARX_CMP_NOT_EQUAL: return c != 0;
    case ARX_CMP_GREATER: return c > 0;
    case ARX_CMP_GREATER_EQUAL: return c >= 0;
    case ARX_CMP_LESS: return c < 0;
    default: return c <= 0;
  }
}

// three-way order of two 8-byte pieces that differ, first byte most significant
__device__ __forceinline__ int order8(uint64_t a, uint64_t b) { return __builtin_bswap64(a) < __builtin_bswap64(b) ? -1 : 1; }

// Consecutive 8-byte pieces of the bytes at p (any alignment) out of aligned words: a word is loaded once, and only if it
// holds a referenced byte.
struct Stream8 {
  const uint64_t* wp;
  uint64_t cur;   // *wp
  int sh;         // bits of cur below the next piece
  __device__ __forceinline__ explicit Stream8(const uint8_t* p) {   // at least one byte at p is referenced
    const uint64_t addr = reinterpret_cast<uint64_t>(p);
    wp = reinterpret_cast<const uint64_t*>(addr & ~uint64_t(7));
    sh = static_cast<int>(addr & 7) * 8;
    cur = *wp;
  }
  // the next piece, of whose bytes the first rem >= 1 are referenced (the others are unspecified)
  __device__ __forceinline__ uint64_t next(int64_t rem) {
    uint64_t w = cur >> sh;
    if (rem > 8 - (sh >> 3)) {   // the following word holds a referenced byte
      cur = *++wp;
      if (sh != 0) w |= cur << (64 - sh);
    }
    return w;
  }
};

// three-way order of a[0, la) and b[0, lb) by one lane; `lengths_decide`: unequal lengths answer without a read
__device__ __forceinline__ int lane_compare(const uint8_t* a, int64_t la, const uint8_t* b, int64_t lb, bool lengths_decide) {
  const int by_length = la < lb ? -1 : (la > lb ? 1 : 0);
  const int64_t common = la < lb ? la : lb;
  if (common == 0 || (lengths_decide && by_length != 0)) return by_length;
  Stream8 sa(a), sb(b);
  for (int64_t k = 0; k < common; k += 8) {
    const int64_t rem = common - k;
    const uint64_t mask = rem >= 8 ? ~uint64_t(0) : ((uint64_t(1) << (8 * rem)) - 1);
    const uint64_t wa = sa.next(rem) & mask, wb = sb.next(rem) & mask;
    if (wa != wb) return order8(wa, wb);
  }
  return by_length;
}

// the full-byte mask of the bytes [from, to) of a 64-bit word (clamped as byte_range_bit7)
__device__ __forceinline__ uint64_t byte_range_mask(int64_t from, int64_t to) { return (byte_range_bit7(from, to) >> 7) * 0xFF; }

struct Granule {
  uint64_t lo, hi;
};
// the aligned granule at address g if it holds a byte of [s, e) (addresses), else zeros without a load
__device__ __forceinline__ Granule load_granule(uint64_t g, uint64_t s, uint64_t e) {
  Granule r{0, 0};
  if (g + 16 > s && g < e) {
    const uint4 q = *reinterpret_cast<const uint4*>(g);
    r.lo = q.x | (static_cast<uint64_t>(q.y) << 32);
    r.hi = q.z | (static_cast<uint64_t>(q.w) << 32);
  }
  return r;
}

// three-way order of a[0, la) and b[0, lb) by one wave: every argument is wave-uniform, all lanes call and all return
// the same value
__device__ __forceinline__ int wave_compare(const uint8_t* a, int64_t la, const uint8_t* b, int64_t lb, bool lengths_decide) {
  const int by_length = la < lb ? -1 : (la > lb ? 1 : 0);
  const int64_t common = la < lb ? la : lb;
  if (common == 0 || (lengths_decide && by_length != 0)) return by_length;
  const int lane = lane_id();
  const uint64_t a0 = reinterpret_cast<uint64_t>(a), b0 = reinterpret_cast<uint64_t>(b);
  const uint64_t a_end = a0 + static_cast<uint64_t>(common), b_end = b0 + static_cast<uint64_t>(common);
  const uint64_t ga = a0 & ~uint64_t(15);               // the left row's first granule; its first byte is row position p0
  const int64_t p0 = -static_cast<int64_t>(a0 & 15);    // -15 .. 0
  const uint64_t bp = b0 + static_cast<uint64_t>(p0);   // where position p0 would lie on the right (may precede its row)
  const uint64_t gb = bp & ~uint64_t(15);
  const int d = static_cast<int>(bp & 15);              // the right row's bytes start d bytes into its granule
  for (int64_t step = 0; p0 + step < common; step += 16 * kWave) {
    const int64_t p = p0 + step + 16 * lane;            // the row position of this lane's first byte
    const uint64_t off = static_cast<uint64_t>(step) + 16 * static_cast<uint64_t>(lane);
    const Granule x = load_granule(ga + off, a0, a_end);
    const Granule y = load_granule(gb + off, b0, b_end);
    Granule z{0, 0};                                    // the right row's granule after y
    if (d != 0) {                                       // (wave-uniform)
      z.lo = __shfl_down(y.lo, 1, 64);
      z.hi = __shfl_down(y.hi, 1, 64);
      if (lane == kWave - 1) z = load_granule(gb + off + 16, b0, b_end);
    }
    // 16 bytes from byte d of y:z
    uint64_t w0 = y.lo, w1 = y.hi, w2 = z.lo;
    int s = d;
    if (s >= 8) {
      w0 = y.hi;
      w1 = z.lo;
      w2 = z.hi;
      s -= 8;
    }
    if (s != 0) {
      w0 = (w0 >> (8 * s)) | (w1 << (64 - 8 * s));
      w1 = (w1 >> (8 * s)) | (w2 << (64 - 8 * s));
    }
    // the bytes of this granule inside the common length: positions [p, p + 16) cut to [0, common)
    const int64_t from = p < 0 ? -p : 0, to = common - p;   // (to <= 0 for a lane past the end: empty masks)
    const uint64_t m_lo = byte_range_mask(from, to), m_hi = byte_range_mask(from - 8, to - 8);
    const uint64_t xl = x.lo & m_lo, xh = x.hi & m_hi, yl = w0 & m_lo, yh = w1 & m_hi;
    const bool differs = xl != yl || xh != yh;
    const uint64_t who = __ballot(differs);
    if (who != 0) {                                     // (wave-uniform) the first lane that differs holds the order
      const int src = __ffsll(static_cast<unsigned long long>(who)) - 1;
      const int mine = xl != yl ? order8(xl, yl) : order8(xh, yh);
      return __shfl(mine, src, 64);
    }
  }
  return by_length;
}

// one side of a call: a column, or (offsets == nullptr) the literal data[0, n_or_len)
template <typename O>
struct Side {
  Bits valid;
  const O* offsets;
  const uint8_t* data;
  int64_t literal_length;
};

// the row `row` of a side: its first byte and its length
template <typename O>
__device__ __forceinline__ void side_row(const Side<O>& s, const uint8_t* literal, int64_t row, const uint8_t** p, int64_t* len) {
  if (s.offsets == nullptr) {
    *p = literal;
    *len = s.literal_length;
  } else {
    const int64_t begin = s.offsets[row];
    *p = s.data + begin;
    *len = static_cast<int64_t>(s.offsets[row + 1]) - begin;
  }
}

// the literal of this workgroup if the right side is one (the left side never is: the mirrored op)
template <typename O>
__device__ __forceinline__ const uint8_t* stage_literal(uint64_t* s_lit, const Side<O>& right) {
  if (right.offsets != nullptr || right.literal_length == 0) return right.data;   // (uniform)
  return stage_pattern(s_lit, right.data, right.literal_length);
}

template <typename O>
__global__ __launch_bounds__(kBlock) void compare_rows_kernel(int op, Side<O> left, Side<O> right, int64_t n, uint64_t* __restrict__ out_bits) {
  __shared__ uint64_t s_lit[kPatternLdsCap / 8] __attribute__((aligned(16)));
  const uint8_t* literal = stage_literal(s_lit, right);
  const bool lengths_decide = op == ARX_CMP_EQUAL || op == ARX_CMP_NOT_EQUAL;
  const int lane = lane_id();
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kBlock; base < n; base += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t row = base + threadIdx.x;
    const bool ok = ((load_word(left.valid, row >> 6) & load_word(right.valid, row >> 6)) >> lane) & 1;   // 0 past the end
    bool hit = false;
    if (ok) {
      const uint8_t *a, *b;
      int64_t la, lb;
      side_row(left, nullptr, row, &a, &la);
      side_row(right, literal, row, &b, &lb);
      hit = answer(op, lane_compare(a, la, b, lb, lengths_decide));
    }
    const uint64_t word = __ballot(hit);
    if (row < n && lane == 0) out_bits[row >> 6] = word;
  }
}

template <typename O>
__global__ __launch_bounds__(kBlock) void compare_waves_kernel(int op, Side<O> left, Side<O> right, int64_t n, uint64_t* __restrict__ out_bits) {
  __shared__ uint64_t s_lit[kPatternLdsCap / 8] __attribute__((aligned(16)));
  const uint8_t* literal = stage_literal(s_lit, right);
  const bool lengths_decide = op == ARX_CMP_EQUAL || op == ARX_CMP_NOT_EQUAL;
  const int lane = lane_id();
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t base = wave * kWave; base < n; base += nwaves * kWave) {
    const uint64_t ok = load_word(left.valid, base >> 6) & load_word(right.valid, base >> 6);   // the step's 64 pairs (0 past the end)
    bool hit = false;
    for (uint64_t todo = ok; todo != 0; todo &= todo - 1) {         // (wave-uniform, and so are the pair's offsets)
      const int i = __ffsll(static_cast<unsigned long long>(todo)) - 1;
      const uint8_t *a, *b;
      int64_t la, lb;
      side_row(left, nullptr, base + i, &a, &la);
      side_row(right, literal, base + i, &b, &lb);
      const int c = wave_compare(a, la, b, lb, lengths_decide);
      if (lane == i) hit = answer(op, c);
    }
    const uint64_t word = __ballot(hit);
    if (lane == 0) out_bits[base >> 6] = word;
  }
}

template <typename O>
Side<O> side_of(const ArxBinarySpan* span, const void* literal, int64_t literal_length, int64_t n) {
  Side<O> s;
  if (span == nullptr) {
    s.valid = make_bits(nullptr, 0, n);
    s.offsets = nullptr;
    s.data = static_cast<const uint8_t*>(literal);
    s.literal_length = literal_length;
  } else {
    const Column c = column_of(span, static_cast<int>(sizeof(O)));
    s.valid = c.valid;
    s.offsets = static_cast<const O*>(c.offsets);
    s.data = c.data;
    s.literal_length = 0;
  }
  return s;
}

template <typename O>
int compare_launch(int op, const ArxBinarySpan* left, const ArxBinarySpan* right, const void* literal, int64_t literal_length, int64_t n,
                   bool waves, void* out_bits, hipStream_t st) {
  if (left == nullptr) {   // literal x array: array x literal under the mirrored op
    static const int kMirrored[] = {ARX_CMP_EQUAL, ARX_CMP_NOT_EQUAL, ARX_CMP_LESS, ARX_CMP_LESS_EQUAL, ARX_CMP_GREATER, ARX_CMP_GREATER_EQUAL};
    op = kMirrored[op];
    std::swap(left, right);
  }
  const Side<O> l = side_of<O>(left, literal, literal_length, n), r = side_of<O>(right, literal, literal_length, n);
  if (waves) {
    hipLaunchKernelGGL(compare_waves_kernel<O>, dim3(waves_grid(n, kWave)), dim3(kBlock), 0, st, op, l, r, n, static_cast<uint64_t*>(out_bits));
    ARX_CHECK_LAUNCH("compare_waves_kernel");
    g_compare_wave_launches.fetch_add(1, std::memory_order_relaxed);
  } else {
    hipLaunchKernelGGL(compare_rows_kernel<O>, dim3(rows_grid(n)), dim3(kBlock), 0, st, op, l, r, n, static_cast<uint64_t*>(out_bits));
    ARX_CHECK_LAUNCH("compare_rows_kernel");
    g_compare_row_launches.fetch_add(1, std::memory_order_relaxed);
  }
  return ARX_OK;
}

}  // namespace

static const CounterRow kStringCompareCounters[] = {
    {"string_compare_row_launches", &g_compare_row_launches},
    {"string_compare_wave_launches", &g_compare_wave_launches},
};
CounterTable string_compare_counters() { return counter_table(kStringCompareCounters); }

}  // namespace arx

using namespace arx;

extern "C" {

int arx_compare_binary(int op, const ArxBinarySpan* left, const ArxBinarySpan* right, int offset_width, const void* literal,
                       int64_t literal_length, int64_t data_bytes_hint, int path, void* out_bits, void* stream) {
  if (left == nullptr && right == nullptr) {
    set_error("compare_binary: both sides are NULL (a literal with a literal has no device kernel)");
    return ARX_INVALID;
  }
  if (op < ARX_CMP_EQUAL || op > ARX_CMP_LESS_EQUAL) {
    set_error("compare_binary: op %d is not 0 (equal) .. 5 (less_equal)", op);
    return ARX_INVALID;
  }
  int rc = check_path("compare_binary", path);
  if (rc != ARX_OK) return rc;
  rc = check_common("compare_binary", left != nullptr ? left : right, offset_width);
  if (rc == ARX_OK && left != nullptr && right != nullptr) rc = check_common("compare_binary", right, offset_width);
  if (rc != ARX_OK) return rc;
  if (left != nullptr && right != nullptr && left->length != right->length) {
    set_error("compare_binary: unequal lengths %lld and %lld", static_cast<long long>(left->length), static_cast<long long>(right->length));
    return ARX_INVALID;
  }
  const bool has_literal = left == nullptr || right == nullptr;
  if (has_literal && (literal_length < 0 || (literal == nullptr && literal_length > 0))) {
    set_error("compare_binary: negative literal_length %lld, or a NULL literal of that length", static_cast<long long>(literal_length));
    return ARX_INVALID;
  }
  const int64_t n = (left != nullptr ? left : right)->length;
  if (n == 0) return ARX_OK;
  if (out_bits == nullptr || (left != nullptr && left->offsets == nullptr) || (right != nullptr && right->offsets == nullptr)) {
    set_error("compare_binary: NULL out_bits or NULL offsets");
    return ARX_INVALID;
  }
  int64_t pair_bytes = mean_bytes(data_bytes_hint, n);
  if (has_literal && pair_bytes >= 0) pair_bytes = 2 * std::min(pair_bytes, literal_length);
  const bool waves = take_waves(path, pair_bytes, kWavesPathMeanPair);
  return with_offset_type(offset_width, [&](auto o) {
    return compare_launch<decltype(o)>(op, left, right, literal, literal_length, n, waves, out_bits, as_stream(stream));
  });
}

}  // extern "C"

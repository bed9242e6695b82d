// binary_join_element_wise on utf8 / binary columns and their large forms: the reference's BinaryJoinElementWise
// (compute/kernels/scalar_string_ascii.cc) under JoinOptions{null_handling, null_replacement}.  Output row i is
// v_1[i], sep[i], v_2[i], ..., sep[i], v_k[i].  Bytes are bytes: no UTF-8 awareness, '\0' and 0xff are ordinary bytes.
// The first row-wise string kernel here with more than one variable-length input, and whose output has a validity of its
// own: a null separator makes the row null in every mode; emit_null: so does a null value; replace: a null value
// contributes the replacement; skip: a null value is left out together with one separator.
// NOT the reference's: under skip a row whose values are all null (separator valid) is the empty string, valid; Arrow
// 25.0.0 drops such a row from its result (include/arrow_amd.h).
//
// Operands: each of the k values and the separator is a column, a literal (a device pointer and a length) or a null
// literal.  They travel to both kernels BY VALUE, as one table of descriptors in the kernel arguments: 40 bytes each,
// ARX_JOIN_MAX_OPERANDS = 32 of them with the separator, 1.3 KiB of the 4 KiB a launch takes.
//
// Two calls, since the output size depends on the validity bits (binary_scan_copy.h):
//   arx_binary_join_offsets  one lane per output row reads the k + 1 offset pairs and validity bits of its row and no
//       data byte; it writes the row's length (64-bit arithmetic) into the workspace's second part — not into out_offsets,
//       which a refused total therefore leaves untouched —, the output validity as one ballot word per 64 rows, adds the
//       lengths of every kBinRows rows into the workspace's 64-bit sums (one atomic a wave) and the null rows into the
//       8-byte word behind the lengths (one atomic a wave of the grid), scans (bin_scan_lengths) and returns the total
//       and the null count;
//   arx_binary_join_data     output-centric, as bin_copy_kernel: a workgroup owns kJoinChunk consecutive output bytes,
//       finds its first and last row by binary search in out_offsets and stages their offsets in LDS (up to kJoinStage
//       rows; more are searched where they lie).  A lane owns one aligned 16-byte granule of the output a step: it finds
//       the row of its first byte by binary search, re-derives the row's pieces (value, separator, value, ...) from the
//       operands' offsets and validity bits exactly as the lengths pass did, skips the pieces before its granule and
//       gathers the granule from the pieces that overlap it, 8 bytes a read (load_bytes8: aligned words, any source
//       alignment), moving on to the following rows while the granule is not full.  One aligned 16-byte store a granule;
//       byte stores only where a granule crosses an end of its chunk or of the output.  The work per output byte is a
//       search over the chunk's rows and a walk over at most 2 k - 1 pieces, whatever the row lengths: a 1 MiB row among
//       short ones is written by 64 workgroups.
//
// Literals (separator, replacement, literal values): up to kPatternLdsCap bytes each they are staged once per workgroup
// in LDS (stage_pattern, string_rows.h) while a pool of kJoinLdsPool bytes has room; a longer one, or one the pool has
// no room for, is read where it lies.
//
// Granule rule (as string_replace.hip): a load touches only an aligned 8-byte piece that holds at least one referenced
// byte of a valid row, or of a literal.  A null row's bytes are never read, whatever its offsets span.
#include "string_rows.h"

#include <type_traits>

namespace arx {

namespace {

constexpr int kJoinChunk = 16384;      // output bytes a workgroup of the data call owns
constexpr int kJoinStage = 2048;       // rows of a chunk whose out offsets are staged in LDS
constexpr int kJoinLdsPool = 4096;     // LDS bytes for the staged literals of a call
constexpr int kJoinReplacement = ARX_JOIN_MAX_OPERANDS;   // the replacement's slot among the staged literals

std::atomic<int64_t> g_join_launches{0};

// One operand as the kernels see it.
struct JoinOp {
  const void* offsets;     // column: element 0 of the logical array
  const uint8_t* data;     // column: the data buffer; literal: its bytes
  const uint64_t* vbase;   // column: the aligned word that holds the first validity bit, or NULL (no nulls)
  int64_t len;             // literal: its length
  int32_t vshift;          // column: the position of the first validity bit inside vbase[0]
  int32_t kind;            // ARX_JOIN_*
};
// What both kernels take by value: op[0, k) the values, op[k] the separator.
struct JoinTable {
  JoinOp op[ARX_JOIN_MAX_OPERANDS];
  const uint8_t* rep;      // the null replacement (device)
  int64_t rep_len;
  int64_t n;               // rows
  int32_t k;
  int32_t mode;            // ARX_JOIN_EMIT_NULL / _SKIP / _REPLACE
};
static_assert(sizeof(JoinOp) == 40 && sizeof(JoinTable) <= 2048, "the table is a kernel argument");

__device__ __forceinline__ bool op_valid(const JoinOp& o, int64_t row) {
  if (o.kind != ARX_JOIN_COLUMN) return o.kind == ARX_JOIN_LITERAL;
  if (o.vbase == nullptr) return true;
  const int64_t bit = o.vshift + row;
  return (o.vbase[bit >> 6] >> (bit & 63)) & 1;
}

template <typename O>
__device__ __forceinline__ int64_t op_len(const JoinOp& o, int64_t row) {
  if (o.kind != ARX_JOIN_COLUMN) return o.len;
  const O* off = static_cast<const O*>(o.offsets);
  return static_cast<int64_t>(off[row + 1]) - static_cast<int64_t>(off[row]);
}

// step one: lens[row] = the output row's length, bit row of out_validity, sums[row / kBinRows] += the length,
// *null_count += the null rows
template <typename O>
__global__ __launch_bounds__(kBlock) void join_lengths_kernel(JoinTable t, O* __restrict__ lens, uint64_t* __restrict__ out_validity,
                                                              unsigned long long* __restrict__ null_count,
                                                              unsigned long long* __restrict__ sums) {
  const int lane = lane_id();
  const JoinOp& sep = t.op[t.k];
  unsigned long long nulls = 0;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kBlock; base < t.n; base += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t row = base + threadIdx.x;
    bool ok = row < t.n && op_valid(sep, row);
    int64_t len = 0;
    if (ok) {
      int64_t kept = 0;
      for (int j = 0; j < t.k; ++j) {
        if (op_valid(t.op[j], row)) {
          len += op_len<O>(t.op[j], row);
          ++kept;
        } else if (t.mode == ARX_JOIN_REPLACE) {
          len += t.rep_len;
          ++kept;
        } else if (t.mode == ARX_JOIN_EMIT_NULL) {
          ok = false;
          break;
        }
      }
      len = ok ? len + (kept > 1 ? (kept - 1) * op_len<O>(sep, row) : 0) : 0;
    }
    if (row < t.n) lens[row] = static_cast<O>(len);
    const uint64_t bal = __ballot(ok);
    const uint64_t total = wave_reduce_sum_u64(static_cast<uint64_t>(len));
    if (lane == 0 && row < t.n) {                                    // (row: the first of the wave's 64)
      out_validity[row >> 6] = bal;
      const int64_t rows = t.n - row < kWave ? t.n - row : kWave;
      nulls += static_cast<unsigned long long>(rows - __popcll(bal));
      if (total != 0) atomicAdd(&sums[row / kBinRows], static_cast<unsigned long long>(total));
    }
  }
  if (lane == 0 && nulls != 0) atomicAdd(null_count, nulls);
}

// step two: the bytes [blockIdx.x kJoinChunk, + kJoinChunk) of the output
template <typename O>
__global__ __launch_bounds__(kBlock) void join_write_kernel(JoinTable t, const O* __restrict__ out_offsets, int64_t total,
                                                            uint8_t* __restrict__ out) {
  __shared__ uint64_t s_pool[kJoinLdsPool / 8];
  __shared__ const uint8_t* s_lit[ARX_JOIN_MAX_OPERANDS + 1];   // literal operand j (and the replacement): staged, or where it lies
  __shared__ int64_t s_off[kJoinStage + 1];
  const int tid = threadIdx.x;
  int used = 0;                                                     // words of the pool taken (uniform)
  for (int j = 0; j <= t.k + 1; ++j) {
    const bool is_rep = j == t.k + 1;
    if (!is_rep && t.op[j].kind != ARX_JOIN_LITERAL) continue;
    const uint8_t* p = is_rep ? t.rep : t.op[j].data;
    const int64_t m = is_rep ? t.rep_len : t.op[j].len;
    const int words = static_cast<int>((m + 7) >> 3);
    if (m > 0 && m <= kPatternLdsCap && used + words <= kJoinLdsPool / 8) {
      p = stage_pattern(s_pool + used, p, m);
      used += words;
    }
    if (tid == 0) s_lit[is_rep ? kJoinReplacement : j] = p;
  }
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * kJoinChunk;
  const int64_t b1 = b0 + kJoinChunk < total ? b0 + kJoinChunk : total;
  const int64_t rlo = bin_row_of<O>(out_offsets, t.n, b0, 0);
  const int64_t rhi = bin_row_of<O>(out_offsets, t.n, b1 - 1, 0);
  const bool staged = rhi - rlo < kJoinStage;
  if (staged) {
    for (int64_t i = tid; i <= rhi - rlo + 1; i += kBlock) s_off[i] = static_cast<int64_t>(out_offsets[rlo + i]);
  }
  __syncthreads();
  auto off = [&](int64_t r) -> int64_t { return staged ? s_off[r - rlo] : static_cast<int64_t>(out_offsets[r]); };
  const JoinOp& sep = t.op[t.k];
  const int64_t q0 = b0 - static_cast<int64_t>((reinterpret_cast<uint64_t>(out) + static_cast<uint64_t>(b0)) & 15);
  for (int64_t q = q0 + 16 * tid; q < b1; q += 16 * kBlock) {
    const int64_t first = q > b0 ? q : b0;
    const int64_t last = q + 16 < b1 ? q + 16 : b1;
    if (first >= last) continue;
    int64_t lo = rlo, hi = rhi + 1;                                 // off(lo) <= first < off(hi)
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (off(mid) <= first) lo = mid; else hi = mid;
    }
    uint64_t w0 = 0, w1 = 0;                                        // the granule's bytes
    int64_t pos = first;                                            // the next output byte to gather
    for (int64_t r = lo; pos < last && r <= rhi; ++r) {
      const int64_t row_end = off(r + 1);
      if (row_end <= pos) continue;                                 // an empty or null row
      // a row that holds bytes is valid: its separator is, and under emit_null so is every value
      int64_t cur = off(r);                                         // where the piece at hand begins in the output
      // out[cur, cur + len) = src[0, len): the part of it inside [pos, last) goes into the granule
      auto piece = [&](const uint8_t* src, int64_t len) {
        const int64_t end = cur + len;
        if (end > pos && pos < last) {
          const int64_t e = end < last ? end : last;
          const uint8_t* p = src + (pos - cur);
          for (int64_t c = pos; c < e; c += 8) {
            const int64_t nb = e - c < 8 ? e - c : 8;
            const uint64_t w = load_bytes8(p + (c - pos), nb);
            const int at = static_cast<int>(c - q);                 // 0 .. 15, at + nb <= 16
            if (at < 8) {
              w0 |= w << (8 * at);
              if (at > 0 && at + nb > 8) w1 |= w >> (64 - 8 * at);
            } else {
              w1 |= w << (8 * (at - 8));
            }
          }
          pos = e;
        }
        cur = end;
      };
      const uint8_t* sep_src = nullptr;
      int64_t sep_len = sep.len;
      if (sep.kind == ARX_JOIN_COLUMN) {
        const int64_t s = static_cast<const O*>(sep.offsets)[r];
        sep_len = static_cast<int64_t>(static_cast<const O*>(sep.offsets)[r + 1]) - s;
        sep_src = sep.data + s;
      } else {
        sep_src = s_lit[t.k];
      }
      bool emitted = false;
      for (int j = 0; j < t.k && pos < last; ++j) {
        const JoinOp& v = t.op[j];
        const uint8_t* src;
        int64_t len;
        if (t.mode == ARX_JOIN_EMIT_NULL || op_valid(v, r)) {
          if (v.kind == ARX_JOIN_COLUMN) {
            const int64_t s = static_cast<const O*>(v.offsets)[r];
            len = static_cast<int64_t>(static_cast<const O*>(v.offsets)[r + 1]) - s;
            src = v.data + s;
          } else {
            len = v.len;
            src = s_lit[j];
          }
        } else if (t.mode == ARX_JOIN_REPLACE) {
          len = t.rep_len;
          src = s_lit[kJoinReplacement];
        } else {
          continue;                                                 // skip: the value and one separator are left out
        }
        if (emitted) piece(sep_src, sep_len);
        piece(src, len);
        emitted = true;
      }
      if (pos < row_end && pos < last) pos = row_end < last ? row_end : last;   // (the pieces make up the row: not reached)
    }
    if (first == q && last == q + 16) {
      *reinterpret_cast<uint4*>(out + q) = make_uint4(static_cast<uint32_t>(w0), static_cast<uint32_t>(w0 >> 32), static_cast<uint32_t>(w1),
                                                      static_cast<uint32_t>(w1 >> 32));
    } else {
      for (int64_t c = first; c < last; ++c) {
        const int at = static_cast<int>(c - q);
        out[c] = static_cast<uint8_t>((at < 8 ? w0 >> (8 * at) : w1 >> (8 * (at - 8))) & 0xFF);
      }
    }
  }
}

// The checks the two calls share, and the table of a checked call.
int make_table(const char* who, const ArxJoinOperand* operands, int num_operands, int64_t length, int offset_width, int null_handling,
               const void* null_replacement, bool replacement_missing, int64_t null_replacement_length, JoinTable* t) {
  if (operands == nullptr) {
    set_error("%s: NULL operands", who);
    return ARX_INVALID;
  }
  ArxBinarySpan shape{};
  shape.length = length;
  const int rc = check_common(who, &shape, offset_width);
  if (rc != ARX_OK) return rc;
  if (num_operands < 1) {
    set_error("%s: %d operands: a call takes at least the separator", who, num_operands);
    return ARX_INVALID;
  }
  if (num_operands > ARX_JOIN_MAX_OPERANDS) {
    set_error("%s: binary_join_element_wise of %d operands: a device call takes %d (ARX_JOIN_MAX_OPERANDS), the separator included", who,
              num_operands, static_cast<int>(ARX_JOIN_MAX_OPERANDS));
    return ARX_NOT_IMPLEMENTED;
  }
  if (null_handling != ARX_JOIN_EMIT_NULL && null_handling != ARX_JOIN_SKIP && null_handling != ARX_JOIN_REPLACE) {
    set_error("%s: null_handling %d is not 0 (emit_null), 1 (skip) or 2 (replace)", who, null_handling);
    return ARX_INVALID;
  }
  if (null_replacement_length < 0) {
    set_error("%s: negative null_replacement_length %lld", who, static_cast<long long>(null_replacement_length));
    return ARX_INVALID;
  }
  if (replacement_missing) {
    set_error("%s: NULL null_replacement of %lld bytes", who, static_cast<long long>(null_replacement_length));
    return ARX_INVALID;
  }
  for (int j = 0; j < num_operands; ++j) {
    const ArxJoinOperand& a = operands[j];
    JoinOp& o = t->op[j];
    o = JoinOp{};
    o.kind = a.kind;
    if (a.kind == ARX_JOIN_COLUMN) {
      if (a.column.length != length) {
        set_error("%s: operand %d is a column of %lld rows in a call of %lld: operand columns are of one length", who, j,
                  static_cast<long long>(a.column.length), static_cast<long long>(length));
        return ARX_INVALID;
      }
      if (length > 0 && a.column.offsets == nullptr) {
        set_error("%s: NULL offsets of operand %d", who, j);
        return ARX_INVALID;
      }
      const Column c = column_of(&a.column, offset_width);
      o.offsets = c.offsets;
      o.data = c.data;
      o.vbase = c.valid.base;
      o.vshift = c.valid.shift;
    } else if (a.kind == ARX_JOIN_LITERAL) {
      if (a.literal_length < 0) {
        set_error("%s: negative literal_length %lld of operand %d", who, static_cast<long long>(a.literal_length), j);
        return ARX_INVALID;
      }
      if (a.literal == nullptr && a.literal_length > 0) {
        set_error("%s: NULL literal of %lld bytes (operand %d)", who, static_cast<long long>(a.literal_length), j);
        return ARX_INVALID;
      }
      o.data = static_cast<const uint8_t*>(a.literal);
      o.len = a.literal_length;
    } else if (a.kind != ARX_JOIN_NULL) {
      set_error("%s: kind %d of operand %d is not 0 (column), 1 (literal) or 2 (null)", who, a.kind, j);
      return ARX_INVALID;
    }
  }
  t->rep = static_cast<const uint8_t*>(null_replacement);
  t->rep_len = null_replacement_length;
  t->n = length;
  t->k = num_operands - 1;
  t->mode = null_handling;
  return ARX_OK;
}

}  // namespace

static const CounterRow kStringJoinCounters[] = {
    {"string_join_launches", &g_join_launches},
};
CounterTable string_join_counters() { return counter_table(kStringJoinCounters); }

}  // namespace arx

using namespace arx;

extern "C" {

size_t arx_binary_join_workspace_bytes(int64_t length, int offset_width) {
  return bin_workspace_bytes(length, offset_width == 8 ? 8 : 4);
}

int arx_binary_join_offsets(const ArxJoinOperand* operands, int num_operands, int64_t length, int offset_width, int null_handling,
                            int64_t null_replacement_length, void* ws, size_t ws_bytes, void* out_offsets, void* out_validity,
                            int64_t* out_null_count, int64_t* out_total_bytes, void* stream) {
  const char* who = "binary_join_offsets";
  if (out_offsets == nullptr || out_validity == nullptr || out_null_count == nullptr || out_total_bytes == nullptr) {
    set_error("%s: NULL out_offsets, out_validity, out_null_count or out_total_bytes", who);
    return ARX_INVALID;
  }
  JoinTable t;
  int rc = make_table(who, operands, num_operands, length, offset_width, null_handling, nullptr, false, null_replacement_length, &t);
  if (rc != ARX_OK) return rc;
  long long nulls = 0;
  rc = offsets_frame(who, "arx_binary_join_workspace_bytes", length, offset_width, ws, ws_bytes, out_offsets, out_total_bytes,
                     "joining binary arrays element-wise", /*lengths_in_ws=*/true, as_stream(stream),
                     [&](auto* out, auto* lens, unsigned long long* sums, hipStream_t st) {
                       using O = std::remove_pointer_t<decltype(out)>;
                       // the null count: the 8-byte word behind the lengths (the workspace's second part has 64 spare bytes)
                       auto* counter = reinterpret_cast<unsigned long long*>(
                           reinterpret_cast<uint8_t*>(lens) + ((static_cast<size_t>(length) * sizeof(O) + 7) & ~static_cast<size_t>(7)));
                       ARX_HIP(hipMemsetAsync(counter, 0, 8, st));
                       hipLaunchKernelGGL(join_lengths_kernel<O>, dim3(rows_grid(length)), dim3(kBlock), 0, st, t, lens,
                                          static_cast<uint64_t*>(out_validity), counter, sums);
                       ARX_CHECK_LAUNCH("join_lengths_kernel");
                       g_join_launches.fetch_add(1, std::memory_order_relaxed);
                       ARX_HIP(hipMemcpyAsync(&nulls, counter, 8, hipMemcpyDeviceToHost, st));   // (bin_scan_lengths waits)
                       return static_cast<int>(ARX_OK);
                     });
  if (rc == ARX_OK) *out_null_count = nulls;
  return rc;
}

int arx_binary_join_data(const ArxJoinOperand* operands, int num_operands, int64_t length, int offset_width, int null_handling,
                         const void* null_replacement, int64_t null_replacement_length, const void* out_offsets,
                         int64_t total_bytes, void* out_data, void* stream) {
  const char* who = "binary_join_data";
  JoinTable t;
  const int rc = make_table(who, operands, num_operands, length, offset_width, null_handling, null_replacement,
                            null_replacement == nullptr && null_replacement_length > 0, null_replacement_length, &t);
  if (rc != ARX_OK) return rc;
  if (total_bytes < 0) {
    set_error("%s: negative total_bytes %lld", who, static_cast<long long>(total_bytes));
    return ARX_INVALID;
  }
  if (length == 0 || total_bytes == 0) return ARX_OK;
  if (out_offsets == nullptr || out_data == nullptr) {
    set_error("%s: NULL out_offsets or out_data", who);
    return ARX_INVALID;
  }
  const int64_t chunks = ceil_div(total_bytes, kJoinChunk);
  if (chunks > 0x7FFFFFFFll) {
    set_error("%s: %lld output bytes are more than one launch takes", who, static_cast<long long>(total_bytes));
    return ARX_NOT_IMPLEMENTED;
  }
  hipStream_t st = as_stream(stream);
  return with_offset_type(offset_width, [&](auto o) {
    using O = decltype(o);
    hipLaunchKernelGGL(join_write_kernel<O>, dim3(static_cast<unsigned>(chunks)), dim3(kBlock), 0, st, t, static_cast<const O*>(out_offsets),
                       total_bytes, static_cast<uint8_t*>(out_data));
    ARX_CHECK_LAUNCH("join_write_kernel");
    g_join_launches.fetch_add(1, std::memory_order_relaxed);
    return static_cast<int>(ARX_OK);
  });
}

}  // extern "C"

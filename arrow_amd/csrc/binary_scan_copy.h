// The two steps every producer of a variable-length column shares: lengths -> offsets, and the copy of the bytes.
// binary.hip defines them (bin_scan_blocks / bin_offsets / bin_copy, see its head comment); the take of binary.hip and
// the slices of string_slice.hip launch them through these two calls, so there is one scan and one copy kernel.
//
// Contract of the producer's own first kernel: it writes the length of output row i into out_offsets[i], the source
// position of its first byte (an index into the values' data buffer) into src_start[i], and the byte total of every
// kBinRows consecutive rows into sums[i / kBinRows] (64-bit).  The workspace holds both: [sums][src_start].
#pragma once
#include "arx_common.h"

namespace arx {

constexpr int kBinRows = kBlock * 16;  // output rows per workgroup total

// bytes of the sums at the head of the workspace; src_start begins right after them
size_t bin_sums_bytes(int64_t rows);
size_t bin_workspace_bytes(int64_t rows, int offset_width);

// lengths in out_offsets[0, length) + sums -> out_offsets[0, length] (exclusive scan, out_offsets[length] = the total).
// Synchronous: *out_total is read back between the scan of the sums and the scan of the rows.  A total that does not fit
// int32 offsets is ARX_INVALID ("offset overflow while <what>: ...") before any offset is written.  length > 0.
// lens: where the lengths lie when the producer kept them out of out_offsets (string_join.hip keeps them in the
// workspace's second part, so a refused call leaves out_offsets untouched); NULL: in out_offsets itself.
template <typename O>
int bin_scan_lengths(O* out_offsets, int64_t length, long long* sums, const char* what, int64_t* out_total, hipStream_t st,
                     const O* lens = nullptr);

// the row of output byte `pos`: the largest r in [0, m) with out_offsets[r] << shift <= pos (pos < out_offsets[m] << shift);
// shift: see bin_copy_rows
template <typename O>
__device__ __forceinline__ int64_t bin_row_of(const O* __restrict__ out_offsets, int64_t m, int64_t pos, int shift) {
  int64_t lo = 0, hi = m;  // invariant: out_offsets[lo] <= pos < out_offsets[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if ((static_cast<int64_t>(out_offsets[mid]) << shift) <= pos) lo = mid; else hi = mid;
  }
  return lo;
}

// out_data[out_offsets[i], out_offsets[i + 1]) = data[src_start[i] ...) for the `rows` rows; copy_bytes = the total << shift
// (shift: the entries count elements of 2^shift bytes, 0 for binary / utf8).  copy_bytes > 0.  Asynchronous.
template <typename O>
int bin_copy_rows(const uint8_t* data, const O* src_start, const O* out_offsets, int64_t rows, int64_t copy_bytes,
                  uint8_t* out_data, int shift, hipStream_t st);

}  // namespace arx

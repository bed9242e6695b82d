// What the row-wise string kernels share (string_slice.hip, string_trim.hip): the bit-7 byte masks of a 16-byte granule,
// the view of a values column, the grid of a one-lane-per-row launch and the argument checks of their C entry points.
#pragma once
#include "binary_scan_copy.h"

#include <algorithm>
#include <atomic>

namespace arx {

constexpr uint64_t kBit7 = 0x8080808080808080ull;

// bit 7 of the bytes [from, to) of a 64-bit word, 0 <= from, to <= 8 after clamping
__device__ __forceinline__ uint64_t byte_range_bit7(int64_t from, int64_t to) {
  from = from < 0 ? 0 : from;
  to = to > 8 ? 8 : to;
  if (to <= from) return 0;
  const uint64_t below_to = to >= 8 ? ~uint64_t(0) : ((uint64_t(1) << (8 * to)) - 1);
  const uint64_t below_from = (uint64_t(1) << (8 * from)) - 1;   // from < 8 here
  return below_to & ~below_from & kBit7;
}

inline int device_cus() {
  static std::atomic<int> cus{0};
  int c = cus.load(std::memory_order_relaxed);
  if (c == 0) {
    int dev = 0, n = 0;
    c = (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
    cus.store(c, std::memory_order_relaxed);
  }
  return c;
}

// one lane per row, a workgroup strides over what is left
inline unsigned rows_grid(int64_t n) {
  return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, kBlock), static_cast<int64_t>(device_cus()) * 8)));
}

struct Column {
  Bits valid;
  const void* offsets;   // element 0 of the logical array
  const uint8_t* data;
  int64_t n;
};
inline Column column_of(const ArxBinarySpan* values, int offset_width) {
  Column c;
  c.n = values->length;
  c.offsets = reinterpret_cast<const uint8_t*>(values->offsets) + values->offset * offset_width;
  c.data = static_cast<const uint8_t*>(values->data);
  c.valid = make_bits(values->null_count == 0 ? nullptr : values->validity, values->offset, c.n);
  return c;
}

// the checks the calls share; `who` names the call
inline int check_common(const char* who, const ArxBinarySpan* values, int offset_width) {
  if (offset_width != 4 && offset_width != 8) {
    set_error("%s: offset_width %d is not 4 or 8", who, offset_width);
    return ARX_INVALID;
  }
  if (values->length < 0) {
    set_error("%s: negative length %lld of values", who, static_cast<long long>(values->length));
    return ARX_INVALID;
  }
  return ARX_OK;
}
// the workspace of an offsets call: [sums][src_start] of binary_scan_copy.h
inline int check_offsets_workspace(const char* who, const void* ws, size_t ws_bytes, int64_t length, int offset_width) {
  if (ws == nullptr || ws_bytes < bin_workspace_bytes(length, offset_width) || (reinterpret_cast<uint64_t>(ws) & 7) != 0) {
    set_error("%s: ws of %llu bytes is NULL, unaligned or smaller than arx_string_slice_workspace_bytes = %llu", who,
              static_cast<unsigned long long>(ws_bytes), static_cast<unsigned long long>(bin_workspace_bytes(length, offset_width)));
    return ARX_INVALID;
  }
  return ARX_OK;
}

}  // namespace arx

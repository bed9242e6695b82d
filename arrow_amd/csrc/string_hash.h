// The 64-bit hash of a var-width value's bytes, shared by the Grouper's string keys (grouper.hip) and set lookup
// (set_lookup.hip): one definition, so that both hash a string to the same value.
#pragma once
#include "arx_common.h"

namespace arx {

// bytes [pos, pos + 8) of the string data[start, start + len), zero past its end (pos < len, pos a multiple of 8): the one
// or two aligned words that hold them, the second only if it holds a byte of the string
__device__ __forceinline__ uint64_t string_word(const uint8_t* data, int64_t start, int64_t len, int64_t pos) {
  const uint64_t addr = reinterpret_cast<uint64_t>(data) + static_cast<uint64_t>(start + pos);
  const uint64_t* wp = reinterpret_cast<const uint64_t*>(addr & ~uint64_t(7));
  const int sh = static_cast<int>(addr & 7) * 8;
  uint64_t w = wp[0] >> sh;
  const int64_t rem = len - pos;
  if (sh != 0 && (8 - (sh >> 3)) < rem) w |= wp[1] << (64 - sh);
  if (rem < 8) w &= (uint64_t(1) << (8 * rem)) - 1;
  return w;
}

// The hash is a XOR over the string's 8-byte words of a mix of (word, word number), finished with the length: the words
// can be folded in any order, so a lane folds a short string alone and a whole wave folds a long one 512 bytes a step
// (coalesced) — one kernel for columns of any mix of lengths, cost proportional to the bytes.
__device__ __forceinline__ uint64_t string_word_mix(uint64_t w, int64_t k) {
  uint64_t x = (w ^ (static_cast<uint64_t>(k + 1) * 0x9E3779B97F4A7C15ull)) * 0x9FB21C651E98DF25ull;
  x ^= x >> 32;
  return x * 0xD6E8FEB86659FD93ull;
}
__device__ __forceinline__ uint64_t string_hash_finish(uint64_t acc, int64_t len) {
  uint64_t h = acc ^ (static_cast<uint64_t>(len) * 0xC2B2AE3D27D4EB4Full) ^ 0x9E3779B97F4A7C15ull;
  h = (h ^ (h >> 33)) * 0xFF51AFD7ED558CCDull;
  h = (h ^ (h >> 33)) * 0xC4CEB9FE1A85EC53ull;
  return h ^ (h >> 33);
}

}  // namespace arx

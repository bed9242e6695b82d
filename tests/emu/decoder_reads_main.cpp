// Reads past the input of the three byte-stream decoders (inflate, Snappy, LZ4), of the two host walks over untrusted
// varints (arx_rle_scan_runs, arx_delta_scan_miniblocks) and of the kernels they feed — TEST INFRASTRUCTURE ONLY.
//
// The Python tests hand the decoders `blocks + 8 zero bytes`, and guard bytes only catch writes: a read of a few bytes past
// a block is invisible there.  This program is linked against the emulated kernel sources with -fsanitize=address
// (tests/test_parquet.py builds it), copies every case of a corpus file into an allocation of EXACTLY its size — input and
// destination alike — runs the decoder on it and prints the status; a read or write outside either allocation ends the run
// with the sanitizer's report.
//
// Corpus (little-endian): u32 number of cases, then per case u32 kind (0 gzip / zlib page, 1 Snappy block with the LDS
// form, 2 Snappy block with the global form, 3 LZ4 frame, 4 RLE / bit-packed hybrid block, 5 DELTA_BINARY_PACKED stream), u32
// input size, u32 dst_size, the input bytes.
//
// Kind 4: dst_size = n | bit width << 24.  Both passes of arx_rle_scan_runs (count, fill) read the exact-size input and
// fill a run table of exactly the counted runs; arx_rle_decode_u32 writes exactly 4 * n bytes; for widths 1..16
// arx_rle_scan_runs_equals counts the values equal to the first decoded one and arx_rle_decode_equals_bitmap writes exactly
// 8 * ceil(n / 64) bytes.  Prints "scan <rc>" when the walk refuses the block, else "sum <crc32 of the values, the bitmap and
// the 8-byte count>".
// Kind 5: dst_size = n | output byte width << 24.  Both passes of arx_delta_scan_miniblocks read the exact-size input; the
// buffer the kernels see is the bytes the walk consumed, rounded up to 8, plus the 8 readable bytes the header comment of
// arx_delta_decode asks for, and no more; the output is exactly n * width bytes.  Prints "scan <rc>", "total <values the
// stream announces>" when that is not n (a reader stops there: the page header says n), else "sum <crc32 of the output>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/arrow_amd.h"

static uint32_t crc32_of(const void* data, size_t n, uint32_t crc = 0) {   // zlib's crc32 (reflected 0xEDB88320), bit by bit
  const uint8_t* p = static_cast<const uint8_t*>(data);
  crc = ~crc;
  for (size_t i = 0; i < n; ++i) {
    crc ^= p[i];
    for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
  }
  return ~crc;
}

// kind 4 -> true and *sum when the walk accepts the block
static bool hybrid_case(const uint8_t* in, uint32_t n_in, uint32_t packed, int* rc, uint32_t* sum) {
  const int64_t n = packed & 0xFFFFFFu;
  const int bw = static_cast<int>(packed >> 24);
  int64_t nr = 0, ones = 0;
  *rc = arx_rle_scan_runs(in, n_in, bw, n, 0, 0, nullptr, 0, &nr, &ones);
  if (*rc != 0) return false;
  ArxRleRun* runs = static_cast<ArxRleRun*>(malloc(static_cast<size_t>(nr) * sizeof(ArxRleRun)));   // exactly the counted runs
  *rc = arx_rle_scan_runs(in, n_in, bw, n, 0, 0, runs, nr, &nr, nullptr);
  uint32_t* out = static_cast<uint32_t*>(malloc(static_cast<size_t>(n) * 4));
  if (*rc == 0) *rc = arx_rle_decode_u32(in, n_in, runs, nr, bw, n, out, nullptr);
  if (*rc == 0) *sum = crc32_of(out, static_cast<size_t>(n) * 4);
  if (*rc == 0 && bw >= 1 && bw <= 16) {
    const uint32_t equals = out[0];
    const size_t nbits = static_cast<size_t>((n + 63) / 64) * 8;
    uint8_t* bits = static_cast<uint8_t*>(malloc(nbits));
    int64_t count = 0, nr2 = 0;
    *rc = arx_rle_scan_runs_equals(in, n_in, bw, n, equals, 0, 0, nullptr, 0, &nr2, &count);
    if (*rc == 0) *rc = arx_rle_decode_equals_bitmap(in, n_in, runs, nr, bw, n, equals, bits, nullptr);
    if (*rc == 0) {
      uint8_t c[8];
      for (int k = 0; k < 8; ++k) c[k] = static_cast<uint8_t>(static_cast<uint64_t>(count) >> (8 * k));
      *sum = crc32_of(c, 8, crc32_of(bits, nbits, *sum));
    }
    free(bits);
  }
  free(out);
  free(runs);
  return *rc == 0;
}

// kind 5 -> true and *sum when the walk accepts the stream and it holds n values; *total = what it announces
static bool delta_case(const uint8_t* in, uint32_t n_in, uint32_t packed, int* rc, int64_t* total, uint32_t* sum) {
  const int64_t n = packed & 0xFFFFFFu;
  const int width = static_cast<int>(packed >> 24);
  int64_t nmb = 0, vpm = 0, first = 0;
  size_t used = 0;
  *total = n;
  *rc = arx_delta_scan_miniblocks(in, n_in, 0, nullptr, 0, &nmb, &vpm, total, &first, &used);
  if (*rc != 0 || *total != n) return false;
  ArxDeltaMiniblock* mbs = static_cast<ArxDeltaMiniblock*>(malloc(static_cast<size_t>(nmb > 0 ? nmb : 1) * sizeof(ArxDeltaMiniblock)));
  *rc = arx_delta_scan_miniblocks(in, n_in, 0, mbs, nmb, &nmb, &vpm, total, &first, &used);
  const size_t seen = ((used + 7) & ~static_cast<size_t>(7)) + 8;
  uint8_t* bytes = static_cast<uint8_t*>(calloc(seen, 1));                 // (malloc's blocks are 16-byte aligned)
  memcpy(bytes, in, used);
  const size_t ws_bytes = arx_delta_decode_workspace_bytes(n);
  void* ws = malloc(ws_bytes);
  uint8_t* out = static_cast<uint8_t*>(malloc(static_cast<size_t>(n) * width));
  if (*rc == 0) *rc = arx_delta_decode(bytes, mbs, nmb, vpm, first, n, width, ws, ws_bytes, out, nullptr);
  if (*rc == 0) *sum = crc32_of(out, static_cast<size_t>(n) * width);
  free(out);
  free(ws);
  free(bytes);
  free(mbs);
  return *rc == 0;
}

static uint32_t read_u32(FILE* f) {
  uint8_t b[4];
  if (fread(b, 1, 4, f) != 4) { fprintf(stderr, "corpus cut short\n"); exit(2); }
  return b[0] | (b[1] << 8) | (b[2] << 16) | (static_cast<uint32_t>(b[3]) << 24);
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s corpus\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (f == nullptr) { perror(argv[1]); return 2; }
  const uint32_t ncases = read_u32(f);
  for (uint32_t c = 0; c < ncases; ++c) {
    const uint32_t kind = read_u32(f), n_in = read_u32(f), dst_size = read_u32(f);
    uint8_t* in = static_cast<uint8_t*>(malloc(n_in));          // exactly the input: nothing readable behind it
    uint8_t* out = static_cast<uint8_t*>(malloc(kind <= 3 ? dst_size : 0));     // exactly the destination (kinds 4, 5: their own)
    if (n_in != 0 && fread(in, 1, n_in, f) != n_in) { fprintf(stderr, "corpus cut short\n"); return 2; }
    uint32_t status = 77;
    int rc = 0;
    if (kind == 4 || kind == 5) {
      uint32_t sum = 0;
      int64_t total = 0;
      if (kind == 4 ? hybrid_case(in, n_in, dst_size, &rc, &sum) : delta_case(in, n_in, dst_size, &rc, &total, &sum)) {
        printf("%u sum %u\n", c, sum);
      } else if (rc != 0) {
        printf("%u scan %d\n", c, rc);
      } else {
        printf("%u total %lld\n", c, static_cast<long long>(total));
      }
      free(in);
      free(out);
      continue;
    }
    if (kind <= 2) {
      ArxSnappyPage page{0, n_in, dst_size, 0};
      if (kind == 0) {
        rc = arx_gzip_decompress_pages(in, &page, 1, out, &status, nullptr);
      } else {
        arx_set_option("snappy_lds", kind == 1 ? 1 : 0);
        rc = arx_snappy_decompress_pages(in, &page, 1, out, &status, nullptr);
      }
    } else {
      int64_t nb = 0;
      rc = arx_lz4_frame_scan(in, n_in, 0, nullptr, 0, &nb, nullptr);
      if (rc == 0) {
        std::vector<ArxLz4Block> blocks(nb > 0 ? nb : 1);
        rc = arx_lz4_frame_scan(in, n_in, 0, blocks.data(), nb, &nb, nullptr);
        ArxLz4Stream stream{};
        stream.first_block = 0;
        stream.num_blocks = static_cast<uint32_t>(nb);
        stream.dst_offset = 0;
        stream.dst_size = dst_size;
        if (rc == 0) rc = arx_lz4_decompress_streams(in, &stream, blocks.data(), 1, out, &status, nullptr);
      }
    }
    if (rc != 0) {
      printf("%u scan %d\n", c, rc);
    } else {
      printf("%u status %u\n", c, status);
    }
    free(in);
    free(out);
  }
  fclose(f);
  return 0;
}

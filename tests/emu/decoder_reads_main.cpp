// Reads past the input of the three byte-stream decoders (inflate, Snappy, LZ4) — TEST INFRASTRUCTURE ONLY.
//
// The Python tests hand the decoders `blocks + 8 zero bytes`, and guard bytes only catch writes: a read of a few bytes past
// a block is invisible there.  This program is linked against the emulated kernel sources with -fsanitize=address
// (tests/test_parquet.py builds it), copies every case of a corpus file into an allocation of EXACTLY its size — input and
// destination alike — runs the decoder on it and prints the status; a read or write outside either allocation ends the run
// with the sanitizer's report.
//
// Corpus (little-endian): u32 number of cases, then per case u32 kind (0 gzip / zlib page, 1 Snappy block with the LDS
// form, 2 Snappy block with the global form, 3 LZ4 frame), u32 input size, u32 dst_size, the input bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/arrow_amd.h"

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
    uint8_t* out = static_cast<uint8_t*>(malloc(dst_size));     // exactly the destination
    if (n_in != 0 && fread(in, 1, n_in, f) != n_in) { fprintf(stderr, "corpus cut short\n"); return 2; }
    uint32_t status = 77;
    int rc = 0;
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

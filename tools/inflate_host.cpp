// inflate_host.cpp -- the inflate core of the device PNG reader (aivc_amd/csrc/inflate_core.h) as a stand-alone host program, one
// lane wide: the same text the kernel runs, so that the host sanitizers can see its bounds logic at work on valid and damaged
// streams.  Build it with any C++17 compiler, e.g.
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/inflate_host.cpp -o inflate_host
// and run `inflate_host cases.bin results.bin` (tests/test_png_read.py does both).
//     cases.bin    uint32 count, then per case: uint32 source bytes, uint32 bytes expected, the source
//     results.bin  per case: uint32 status (include/aivc_hip_png_read.h: AIVC_INFLATE_*), uint32 bytes produced, uint32 source bytes
//                  consumed, then the destination, `bytes expected` bytes that were 0xA5 before the run
// Every source and destination is a heap block of exactly its size: a read or write one byte outside is the sanitizer's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../aivc_amd/csrc/inflate_core.h"

struct HostEnv {
  static uint32_t lane() { return 0; }
  static uint32_t lanes() { return 1; }
  static void sync() {}
  static uint32_t uniform(uint32_t v) { return v; }
  static uint64_t ballot(bool p) { return p ? 1u : 0u; }
  static uint64_t sum(uint64_t v) { return v; }
};

static bool read_u32(FILE *f, uint32_t &v) { return fread(&v, 4, 1, f) == 1; }

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]);
    return 2;
  }
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  uint32_t count = 0;
  if (!in || !out || !read_u32(in, count)) {
    fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]);
    return 2;
  }
  std::unique_ptr<inflate_core::State> state(new inflate_core::State);
  for (uint32_t k = 0; k < count; ++k) {
    uint32_t n = 0, expect = 0;
    if (!read_u32(in, n) || !read_u32(in, expect) || n >= 1u << 31 || expect >= 1u << 31) {
      fprintf(stderr, "case %u: bad record\n", k);
      return 2;
    }
    uint8_t *src = static_cast<uint8_t *>(malloc(n)), *dst = static_cast<uint8_t *>(malloc(expect));  // (exactly: see above)
    if (n && fread(src, 1, n, in) != n) {
      fprintf(stderr, "case %u: short source\n", k);
      return 2;
    }
    if (expect) memset(dst, 0xA5, expect);
    memset(state.get(), 0x5A, sizeof(inflate_core::State));  // nothing may depend on what an earlier stream left
    uint32_t produced = 0, consumed = 0;
    const uint32_t status = inflate_core::inflate_stream<HostEnv>(*state, src, n, dst, expect, produced, consumed);
    const uint32_t head[3] = {status, produced, consumed};
    fwrite(head, 4, 3, out);
    if (expect) fwrite(dst, 1, expect, out);
    free(src);
    free(dst);
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 2;
}

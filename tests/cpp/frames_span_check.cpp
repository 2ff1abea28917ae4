// frames_span_check.cpp — zh_frame_span (csrc/zh_frames.h) on the host, against the walks that
// tests/test_frames_span.py wrote down from its Python model.  Stand-alone (its own main), meant
// to be built with AddressSanitizer and UBSan: every buffer handed to zh_frame_span is a heap
// allocation exactly as long as the bytes it may read, so a read past the end stops the program.
//
// Input file (little-endian): u32 count, then per vector
//   u32 len | bytes | u32 nframes | nframes x { u64 off, u64 size, u64 fcs, u32 skippable } | u32 status | u64 err_off
// Per vector: the walk from offset 0 must give exactly these frames and this verdict; then every
// frame is cut at every length t below its size, and each cut must fail (and a cut of four bytes
// or more of a first frame with a wrong magic must say so).  A cut is the frame's bytes
// [off, off + t) alone in a heap buffer of t bytes; for a frame over 4 KiB, where that many copies
// would take minutes, only every 97th cut and the first and last 300 get a buffer of their own
// and the others run in one heap copy of the frame whose bytes from t on are poisoned: the
// sanitizer stops a read of them just the same.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zh_frames.h"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#else
#define ASAN_POISON_MEMORY_REGION(p, n) ((void)(p), (void)(n))
#define ASAN_UNPOISON_MEMORY_REGION(p, n) ((void)(p), (void)(n))
#endif

namespace {

struct Reader {
  FILE *f;
  template <typename T> T get() {
    T v{};
    if (fread(&v, sizeof(T), 1, f) != 1) {
      fprintf(stderr, "short input file\n");
      exit(2);
    }
    return v;
  }
};

struct Want {
  uint64_t off, size, fcs;
  uint32_t skippable;
};

int fail(const char *what, unsigned vec, uint64_t at) {
  fprintf(stderr, "vector %u: %s at %llu\n", vec, what, (unsigned long long)at);
  return 1;
}

// zh_frame_span over a copy of exactly n bytes
uint32_t span_exact(const uint8_t *p, uint64_t n, bool first, ZhFrameSpan *s) {
  uint8_t *const h = (uint8_t *)malloc(n ? n : 1);  // (n == 0: one byte that must not be read either way)
  if (n) memcpy(h, p, n);
  uint32_t const st = n ? zh_frame_span(h, n, first, s) : zh_frame_span(h + 1, 0, first, s);
  free(h);
  return st;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  Reader r{fopen(argv[1], "rb")};
  if (!r.f) return 2;
  uint32_t const count = r.get<uint32_t>();
  uint64_t cuts = 0, frames = 0;
  for (uint32_t v = 0; v < count; v++) {
    uint32_t const len = r.get<uint32_t>();
    std::vector<uint8_t> bytes(len);
    if (len && fread(bytes.data(), 1, len, r.f) != len) return 2;
    uint32_t const nf = r.get<uint32_t>();
    std::vector<Want> want(nf);
    for (auto &w : want) {
      w.off = r.get<uint64_t>();
      w.size = r.get<uint64_t>();
      w.fcs = r.get<uint64_t>();
      w.skippable = r.get<uint32_t>();
    }
    uint32_t const status = r.get<uint32_t>();
    uint64_t const err_off = r.get<uint64_t>();

    // ---- the walk, every frame in a buffer that ends where the vector ends
    uint64_t ip = 0, k = 0;
    uint32_t st = ZH_FRAMES_OK;
    while (ip < len) {
      ZhFrameSpan s{};
      st = span_exact(bytes.data() + ip, len - ip, ip == 0, &s);
      if (st != ZH_FRAMES_OK) break;
      if (k >= nf) return fail("a frame too many", v, ip);
      if (want[k].off != ip || want[k].size != s.size || want[k].fcs != s.fcs || want[k].skippable != s.skippable)
        return fail("frame differs from the model", v, ip);
      if (s.size == 0 || s.size > len - ip) return fail("extent outside the buffer", v, ip);
      ip += s.size;
      k++;
    }
    if (k != nf || st != status || (st != ZH_FRAMES_OK && ip != err_off)) return fail("verdict differs from the model", v, ip);
    frames += nf;

    // ---- every cut of every frame (and of the failing tail)
    for (uint32_t i = 0; i <= nf; i++) {
      uint64_t const off = i < nf ? want[i].off : (status ? err_off : len), size = i < nf ? want[i].size : len - off;
      bool const first = off == 0;
      uint8_t *const whole = (uint8_t *)malloc(size ? size : 1);
      if (size) memcpy(whole, bytes.data() + off, size);
      for (uint64_t t = 0; t < size; t++) {
        ZhFrameSpan s{};
        uint32_t c;
        if (size > 4096 && t > 300 && t + 300 < size && t % 97) {
          ASAN_POISON_MEMORY_REGION(whole + t, size - t);
          c = zh_frame_span(whole, t, first, &s);
          ASAN_UNPOISON_MEMORY_REGION(whole + t, size - t);
        } else {
          c = span_exact(bytes.data() + off, t, first, &s);
        }
        cuts++;
        if (c == ZH_FRAMES_OK) return fail("a cut frame passes", v, off + t);
        bool const magic_known = t >= 4 && !zh_frames_is_magic(zh_frames_ld32(bytes.data() + off));
        if ((c == ZH_FRAMES_BAD_MAGIC) != (first && magic_known)) return fail("wrong code for a cut frame", v, off + t);
      }
      free(whole);
    }
  }
  printf("frames span OK: %u vectors, %llu frames, %llu cuts\n", count, (unsigned long long)frames, (unsigned long long)cuts);
  return 0;
}

// adaptive.cpp — C++ driver of include/cuda_zstd_adaptive.h with the reference's call shapes
// (test infrastructure; tests/test_gpu_adaptive_cpp.py checks what it prints against the model).
//
// Buffers: 65536 zero bytes, and 100000 bytes of a linear congruential generator
// (x = 1664525 x + 1013904223 from 12345, byte = x >> 24) whose bytes from 4096 on are 0x41.
// Lines: "R <tag> <status> <level> <strategy> <confidence> <entropy> <repetition> <compressibility>
// <unique> <max_run> <avg_match> <has_patterns> <is_random> <reasoning length>", "L <tag> <status>
// <level>", "C <tag> <status> <compressible> <ratio>", "E <tag> <status>".
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "cuda_zstd_adaptive.h"

using namespace cuda_zstd;
using namespace cuda_zstd::adaptive;

static void print_result(const char *tag, Status st, const AdaptiveResult &r) {
  const DataCharacteristics &c = r.characteristics;
  printf("R %s %d %d %d %.3f %.6f %.6f %.6f %u %u %u %d %d %zu\n", tag, (int)st, r.recommended_level, (int)r.recommended_strategy, r.confidence,
         c.entropy, c.repetition_ratio, c.compressibility, c.unique_bytes, c.max_run_length, c.avg_match_length, (int)c.has_patterns,
         (int)c.is_random, r.reasoning ? strlen(r.reasoning) : (size_t)0);
}

static bool same(const DataCharacteristics &a, const DataCharacteristics &b) {
  return a.entropy == b.entropy && a.repetition_ratio == b.repetition_ratio && a.compressibility == b.compressibility &&
         a.unique_bytes == b.unique_bytes && a.max_run_length == b.max_run_length && a.avg_match_length == b.avg_match_length &&
         a.has_patterns == b.has_patterns && a.is_random == b.is_random;
}

int main() {
  size_t const NZ = 65536, NL = 100000;
  std::vector<unsigned char> lcg(NL);
  unsigned x = 12345u;
  for (size_t i = 0; i < NL; i++) {
    x = 1664525u * x + 1013904223u;
    lcg[i] = i < 4096 ? (unsigned char)(x >> 24) : (unsigned char)0x41;
  }
  unsigned char *d_zero = nullptr, *d_lcg = nullptr;
  hipStream_t stream = nullptr;
  if (hipMalloc((void **)&d_zero, NZ) != hipSuccess || hipMalloc((void **)&d_lcg, NL) != hipSuccess || hipMemset(d_zero, 0, NZ) != hipSuccess ||
      hipMemcpy(d_lcg, lcg.data(), NL, hipMemcpyHostToDevice) != hipSuccess || hipStreamCreate(&stream) != hipSuccess) {
    fprintf(stderr, "device setup failed\n");
    return 2;
  }

  AdaptiveResult r;
  {  // default constructor: BALANCED, 64 KiB sample
    AdaptiveLevelSelector sel;
    Status st = sel.select_level(d_zero, NZ, r);
    print_result("zeros_default", st, r);
    printf("E last_equals_result %d\n", same(sel.get_last_characteristics(), r.characteristics) ? 0 : 1);
    st = sel.select_level(d_lcg, NL, r, stream);
    print_result("lcg_default_stream", st, r);
    sel.set_sample_size(4096);  // only the generator's bytes
    sel.enable_quick_analysis(true);  // no effect
    st = sel.select_level(d_lcg, NL, r, stream);
    print_result("lcg_sample4096", st, r);
    sel.set_preference(AdaptivePreference::RATIO);
    st = sel.select_level(d_zero, NZ, r);
    print_result("zeros_set_ratio", st, r);
    sel.reset_statistics();
    printf("E reset_clears %d\n", same(sel.get_last_characteristics(), DataCharacteristics()) ? 0 : 1);
    // errors leave the status, nothing else
    printf("E null %d\n", (int)sel.select_level(nullptr, NZ, r));
    printf("E zero_size %d\n", (int)sel.select_level(d_zero, 0, r));
  }
  {
    AdaptiveLevelSelector speed(AdaptivePreference::SPEED), ratio(AdaptivePreference::RATIO);
    Status st = speed.select_level(d_zero, NZ, r);
    print_result("zeros_speed", st, r);
    st = ratio.select_level(d_lcg, 4096, r);
    print_result("lcg4096_ratio", st, r);
  }
  int level = -1;
  Status st = select_adaptive_level(d_zero, NZ, level);
  printf("L zeros_free_default %d %d\n", (int)st, level);
  st = select_adaptive_level(d_lcg, 4096, level, AdaptivePreference::SPEED, stream);
  printf("L lcg4096_free_speed %d %d\n", (int)st, level);
  st = analyze_and_select(d_lcg, NL, r, AdaptivePreference::RATIO, stream);
  print_result("lcg_free_ratio", st, r);
  st = analyze_and_select(d_zero, 300, r);
  print_result("zeros300_free", st, r);
  bool comp = false;
  float ratio = 0.0f;
  st = is_compressible(d_zero, NZ, comp, ratio);
  printf("C zeros %d %d %.6f\n", (int)st, (int)comp, ratio);
  st = is_compressible(d_lcg, 4096, comp, ratio, stream);
  printf("C lcg4096 %d %d %.6f\n", (int)st, (int)comp, ratio);
  printf("E free_null %d\n", (int)select_adaptive_level(nullptr, NZ, level));
  printf("E free_zero_size %d\n", (int)analyze_and_select(d_zero, 0, r));
  printf("E compressible_null %d\n", (int)is_compressible(nullptr, 16, comp, ratio));

  (void)hipStreamDestroy(stream);
  (void)hipFree(d_zero);
  (void)hipFree(d_lcg);
  printf("DONE\n");
  return 0;
}

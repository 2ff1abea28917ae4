// zh_adaptive.h — adaptive level selection: the rule shared by the finalize kernel
// (zh_adaptive.hip) and the host entries (zh_host_adaptive.cpp), and the kernels' launch entry.
//
// Statistics of a chunk's first n = min(size, sample_bytes) bytes a[0..n) (DESIGN.md "Adaptive
// level selection"; the reference's selector, src/cuda_zstd_adaptive.cu, restated as exact
// integer definitions):
//   hist[256]        byte counts
//   unique_bytes     non-zero hist entries
//   repeated_pairs   #{ i in [0, n-1) : a[i] == a[i+1] }
//   max_run_length   0 without a repeated pair, else min(longest run of equal bytes, 256)
//   pattern_score    0 for n < 5, else over i in [0, n-4): +1 when a[i]==a[i+2] && a[i+1]==a[i+3],
//                    +2 when i + 8 < n and a[i..i+4) == a[i+4..i+8)
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "cuda_zstd_capi.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZH_AD_HD __host__ __device__ inline
#else
#define ZH_AD_HD inline
#endif

// Per-chunk record of the analysis kernel in the caller's temp buffer: hist[256], then these.
#define ZH_AD_REC_PAIRS 256u
#define ZH_AD_REC_RUN 257u
#define ZH_AD_REC_PATTERN 258u
#define ZH_AD_REC_WORDS 259u
#define ZH_AD_TILE 16384u     // sample bytes of one work item (workgroup)
#define ZH_AD_RUN_CAP 256u    // max_run_length saturates here, which makes it tileable
#define ZH_AD_MAX_SAMPLE 0xFFFFFFFFull  // n is a u32

enum : uint32_t { ZH_AD_HAS_PATTERNS = 1u, ZH_AD_IS_RANDOM = 2u };
// Branch of the rule that gave the level (the index of the reasoning string); EMPTY: a chunk of size 0
enum : int { ZH_AD_RANDOM = 0, ZH_AD_REPETITIVE, ZH_AD_HIGH, ZH_AD_MEDIUM, ZH_AD_LOW, ZH_AD_EMPTY, ZH_AD_BRANCHES };

// One histogram bin's term of -sum p log2 p
ZH_AD_HD float zh_adaptive_entropy_term(uint32_t count, float inv_n) {
  float const p = (float)count * inv_n;
  return count ? -p * log2f(p) : 0.0f;
}

// The level of a branch of the rule under a preference (0 SPEED, 1 BALANCED, 2 RATIO), one byte each
ZH_AD_HD int zh_adaptive_level(int branch, int preference) {
  uint32_t const packed = branch == ZH_AD_RANDOM       ? 0x030301u
                          : branch == ZH_AD_REPETITIVE ? 0x130C06u
                          : branch == ZH_AD_HIGH       ? 0x100905u
                          : branch == ZH_AD_MEDIUM     ? 0x0C0603u
                          : branch == ZH_AD_LOW        ? 0x060301u
                                                       : 0x030303u;
  return (int)((packed >> (8 * preference)) & 0xFFu);
}

// Derived values and the level from the integer statistics and the entropy (fp32): the reference's
// decision tree, evaluated in its order.  preference: 0 SPEED, 1 BALANCED, 2 RATIO.  Returns the
// branch taken.  n == 0: all-zero statistics, level 3.
ZH_AD_HD int zh_adaptive_decide(uint32_t n, uint32_t repeated_pairs, uint32_t max_run_length, uint32_t pattern_score, uint32_t unique_bytes,
                                float entropy, int preference, cuda_zstd_adaptive_stats_t *o) {
  o->sample_size = n;
  o->repeated_pairs = repeated_pairs;
  o->max_run_length = max_run_length;
  o->pattern_score = pattern_score;
  o->unique_bytes = unique_bytes;
  if (n == 0) {
    o->flags = 0;
    o->entropy = o->repetition_ratio = o->compressibility = 0.0f;
    o->level = 3;
    return ZH_AD_EMPTY;
  }
  float const rep = (float)repeated_pairs / (float)n;
  float comp = 0.6f * (1.0f - entropy / 8.0f) + 0.4f * rep;
  comp = comp < 0.0f ? 0.0f : comp > 1.0f ? 1.0f : comp;
  bool const has_patterns = pattern_score > n / 100u;
  bool const is_random = entropy > 7.5f && !has_patterns;
  o->flags = (has_patterns ? ZH_AD_HAS_PATTERNS : 0u) | (is_random ? ZH_AD_IS_RANDOM : 0u);
  o->entropy = entropy;
  o->repetition_ratio = rep;
  o->compressibility = comp;
  int const branch = is_random                                    ? ZH_AD_RANDOM
                     : (rep > 0.5f || max_run_length > 100u)      ? ZH_AD_REPETITIVE
                     : comp > 0.7f                                ? ZH_AD_HIGH
                     : comp > 0.4f                                ? ZH_AD_MEDIUM
                                                                  : ZH_AD_LOW;
  o->level = zh_adaptive_level(branch, preference);
  return branch;
}

namespace zh {
// Workgroups of the analysis launch: every chunk gets the tiles of a sample that starts up to 15
// bytes into its first 16-byte line.  0: the grid would not fit (the entry returns INVALID).
uint32_t adaptive_grid(size_t num_chunks, size_t sample_bytes);
// Zeroes the records, analyses every chunk and writes d_levels (and d_stats when not null); all on
// `stream`, nothing allocated or synchronised.  d_ptrs null: one chunk, one_ptr / one_size.
// d_temp: num_chunks records of ZH_AD_REC_WORDS u32.
hipError_t adaptive_launch(const void *const *d_ptrs, const size_t *d_sizes, const void *one_ptr, size_t one_size, size_t num_chunks,
                           size_t sample_bytes, int preference, cuda_zstd_adaptive_stats_t *d_stats, int *d_levels, uint32_t *d_temp,
                           hipStream_t stream);
}  // namespace zh

// zh_scan.h — wave64 / workgroup prefix sums shared by the scan kernels (zh_seek.hip,
// zh_dict_train.hip).  Workgroups of ZH_SCAN_THREADS threads.
#pragma once
#include "zh_common.h"

#define ZH_SCAN_THREADS 256u

__device__ __forceinline__ u64 wave_scan_incl64(u64 v) {
  u32 const lane = threadIdx.x & 63u;
#pragma unroll
  for (u32 o = 1; o < 64; o <<= 1) {
    u64 const t = __shfl_up((unsigned long long)v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// Exclusive scan of one u64 per thread over a 256-thread workgroup; total = the workgroup's sum.
// lds: 4 u64 (reusable after the call returns).
__device__ __forceinline__ u64 block_scan_excl64(u64 v, u64 *lds, u64 &total) {
  u32 const tid = threadIdx.x, w = tid >> 6;
  u64 const inc = wave_scan_incl64(v);
  __syncthreads();
  if ((tid & 63u) == 63u) lds[w] = inc;
  __syncthreads();
  u64 base = 0, tot = 0;
#pragma unroll
  for (u32 k = 0; k < ZH_SCAN_THREADS / 64; k++) {
    u64 const s = lds[k];
    base += k < w ? s : 0ull;
    tot += s;
  }
  total = tot;
  return base + inc - v;
}

// zh_adaptive.hip — adaptive level selection: one analysis launch over a whole batch.
//
// zh_adaptive_analyze_kernel: one workgroup (4 waves) per (chunk, 16 KiB tile of its sample);
// chunk pointers and sizes are read on the device.  A tile is cut in "line space": the chunk's
// bytes seen from the 16-byte line its base pointer lies in, so a chunk's bytes sit at
// [mis, mis + n), mis = base & 15, and every 16-byte load is aligned; the (at most two) vectors
// that straddle an end of the sample are assembled byte-wise, so nothing outside [0, n) is read.
// A wave takes 4 KiB as four rows of 64 x 16 bytes, plus a 17-vector extension past its end.  All
// statistics come from those registers in one pass:
//   hist            ds_add into one of 16 sub-histograms of the workgroup, chosen by lane & 15 and
//                   257 words apart, so lanes that meet the same byte value hit 16 different
//                   banks (one sub-histogram per wave, the K1 scan's layout, spent 87 % of its
//                   LDS cycles in bank conflicts on text-like chunks and held the kernel at
//                   twice this time: DESIGN.md); reduced after a barrier into one global atomic
//                   add per non-zero bin
//   repeated_pairs, pattern_score
//                   the lane's 16 bytes against themselves 1, 2 and 4 bytes on (the following 8
//                   bytes come from the next lane by DPP, lane 63's from the next row).  Rows that
//                   lie wholly inside the sample compare whole words and count over the wave on
//                   the scalar unit; edge rows use SWAR byte compares as 16-bit position masks
//                   under a validity mask.  Counts are wave-reduced, one atomic each
//   max_run_length  1 + the longest streak of ones in the a[i]==a[i+1] mask.  Every streak ends
//                   where a lane's mask has its first zero, and starts after the last zero before
//                   it: a max-scan (DPP) of "last zero so far" across the lanes and the rows.
//                   A wave counts streaks from its first byte on (which cannot exceed the true
//                   run) and follows them through the extension, 255 bits past its end: the cap
//                   at 256 makes that exact.  One atomic max per wave.
// zh_adaptive_finalize_kernel: one wave per chunk; entropy by a wave reduction over the 256 bins,
// then zh_adaptive_decide (zh_adaptive.h), the function the host entries use.
#include "zh_adaptive.h"
#include "zh_common.h"

namespace {

constexpr u32 AD_THREADS = 256, AD_WAVES = AD_THREADS / 64;
constexpr u32 AD_ROWS = 4;                                  // 64 x 16-byte rows of a wave
constexpr u32 AD_WAVE_BYTES = AD_ROWS * 64u * 16u;          // 4 KiB
constexpr u32 AD_EXT = ZH_AD_RUN_CAP / 16u;                 // extension vectors whose masks count
constexpr u32 AD_SUB = 16, AD_SUB_STRIDE = 257;              // sub-histograms of a workgroup, words apart
static_assert(AD_WAVES * AD_WAVE_BYTES == ZH_AD_TILE, "four waves cover a tile");
static_assert(AD_SUB * AD_SUB_STRIDE % 4u == 0, "cleared as uint4");

}  // namespace

struct ZhAdBatch {
  const void *const *ptrs;  // null: the single chunk one_ptr / one_size
  const size_t *sizes;
  const void *one_ptr;
  u64 one_size;
  u32 nchunks, tiles, sample;
};

namespace {

__device__ __forceinline__ u32 ad_chunk(const ZhAdBatch &b, u32 c, const u8 *&p) {
  p = (const u8 *)(b.ptrs ? b.ptrs[c] : b.one_ptr);
  u64 const size = b.ptrs ? (u64)b.sizes[c] : b.one_size;
  return (u32)(size < b.sample ? size : (u64)b.sample);
}

// Chunk pointers come out of memory, so the compiler knows no address space for them: say global
typedef const __attribute__((address_space(1))) u8 *ad_gptr;
typedef u32 ad_u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) ad_u32x4 *ad_gvec;

// Line-space bytes [W, W + 16) (W a multiple of 16); bytes outside [lo, hi) read as 0 and are not touched
__device__ __forceinline__ uint4 ad_load(ad_gptr line0, u64 W, u64 lo, u64 hi) {
  if (W >= lo && W + 16u <= hi) {
    ad_u32x4 const v = *(ad_gvec)(line0 + W);
    return make_uint4(v.x, v.y, v.z, v.w);
  }
  u32 d[4] = {0u, 0u, 0u, 0u};
  if (W + 16u > lo && W < hi) {
#pragma unroll
    for (u32 j = 0; j < 16u; j++) {
      u64 const q = W + j;
      if (q >= lo && q < hi) d[j >> 2] |= (u32)line0[q] << (8u * (j & 3u));
    }
  }
  return make_uint4(d[0], d[1], d[2], d[3]);
}

// bit j (0..3) = byte j of a equals byte j of b
__device__ __forceinline__ u32 ad_eq4(u32 a, u32 b) {
  u32 const y = a ^ b;
  u32 t = ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);  // 0x80 in every zero byte, exactly
  t >>= 7;
  return (t | t >> 7 | t >> 14 | t >> 21) & 15u;
}

__device__ __forceinline__ u32 ad_below(u32 k) { return (1u << k) - 1u; }  // k <= 16

// a[i] == a[i+1] for the 16 positions of a vector; d4 = the dword after it
__device__ __forceinline__ u32 ad_pair_mask(uint4 x, u32 d4) {
  return ad_eq4(x.x, __builtin_amdgcn_alignbyte(x.y, x.x, 1)) | ad_eq4(x.y, __builtin_amdgcn_alignbyte(x.z, x.y, 1)) << 4 |
         ad_eq4(x.z, __builtin_amdgcn_alignbyte(x.w, x.z, 1)) << 8 | ad_eq4(x.w, __builtin_amdgcn_alignbyte(d4, x.w, 1)) << 12;
}

__device__ __forceinline__ u32 wave_sum(u32 v) { return lane_value(wave_scan_incl(v), 63u); }

// Longest streak of ones over the masks fed row by row, lanes in order (bit j of lane l of a row =
// bit 16 l + j): `carry` = 1 + the index of the last zero bit so far (0: none; the bit before the
// first counts as zero), `best` = the longest streak that has ended, per lane.
struct AdRuns {
  u32 carry = 0, best = 0;
  __device__ __forceinline__ void row(u32 m, u32 base) {  // base = index of this lane's bit 0
    u32 const nm = ~m & 0xFFFFu;
    u32 inner = 0;
    for (u32 x = m; x; x &= x >> 1) inner++;  // streaks inside the lane
    u32 const sc = wave_scan_max_incl(nm ? base + 32u - (u32)__clz(nm) : 0u);
    u32 const start = max(wave_shr1(sc), carry);  // first bit of the streak that runs into this lane
    u32 const lead = (u32)__builtin_ctz(nm | 0x10000u);  // ones before the lane's first zero
    best = max(best, max(inner, base + lead - start));
    carry = max(carry, lane_value(sc, 63u));
  }
};

}  // namespace

extern "C" __global__ __launch_bounds__(AD_THREADS) void zh_adaptive_analyze_kernel(ZhAdBatch b, u32 *__restrict__ temp) {
  __shared__ __attribute__((aligned(16))) u32 hist[AD_SUB * AD_SUB_STRIDE];
  u32 const chunk = blockIdx.x / b.tiles, tile = blockIdx.x - chunk * b.tiles;
  u32 const tid = threadIdx.x, lane = tid & 63u, wave = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));  // (scalar: row tests branch)
  const u8 *p;
  u32 const n = ad_chunk(b, chunk, p);
  u64 const lo = (u64)((uintptr_t)p & 15u), hi = lo + n;
  u64 const T0 = (u64)tile * ZH_AD_TILE;
  if (T0 >= hi) return;  // (whole workgroup) a tile past the sample, or an empty chunk
  ad_gptr const line0 = (ad_gptr)(p - lo);
  u32 *const rec = temp + (size_t)chunk * ZH_AD_REC_WORDS;

  for (u32 i = tid; i < AD_SUB * AD_SUB_STRIDE / 4u; i += AD_THREADS) ((uint4 *)hist)[i] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();

  u64 const W0 = T0 + (u64)wave * AD_WAVE_BYTES;  // the wave's first line-space byte
  if (W0 < hi) {                                  // (whole wave)
    u32 *const hw = hist + AD_SUB_STRIDE * (lane & (AD_SUB - 1u));
    uint4 x[AD_ROWS + 1];
#pragma unroll
    for (u32 u = 0; u < AD_ROWS; u++) x[u] = ad_load(line0, W0 + 1024u * u + 16u * lane, lo, hi);
    x[AD_ROWS] = lane <= AD_EXT ? ad_load(line0, W0 + AD_WAVE_BYTES + 16u * lane, lo, hi) : make_uint4(0u, 0u, 0u, 0u);
    u32 pairs = 0, score = 0, score_full = 0;  // score_full: wave totals of the full rows (scalar)
    AdRuns runs;
#pragma unroll
    for (u32 u = 0; u <= AD_ROWS; u++) {
      u64 const Wrow = W0 + 1024u * u, W = Wrow + 16u * lane;
      // the 8 bytes after the vector: the next lane's, lane 63's from the next row's lane 0
      u32 d4 = wave_shl1(x[u].x), d5 = wave_shl1(x[u].y);
      if (u < AD_ROWS) {
        u32 const un = u < AD_ROWS ? u + 1u : u;  // (an index inside x[] in the unrolled extension row too)
        u32 const n4 = lane_value(x[un].x, 0u), n5 = lane_value(x[un].y, 0u);
        if (lane == 63u) d4 = n4, d5 = n5;
      }
      u32 const d[6] = {x[u].x, x[u].y, x[u].z, x[u].w, d4, d5};
      // Cross-lane work (the DPP above, the run scan below) stays outside the branch.  With the
      // scan inside, the compiler lowered this uniform branch as a divergent one, and the readlane of
      // the side that no lane takes overwrote the scan's scalar carry: every run came out 256
      u32 m1;
      if (u < AD_ROWS && __builtin_amdgcn_readfirstlane((int)(Wrow >= lo && Wrow + 1024u + 8u <= hi))) {
        // (whole wave) every lane's 24-byte window lies inside the sample: no position masks, and
        // the pattern compares are whole-word compares counted over the wave by the scalar unit.
        // w[q] = the 4 bytes at q; a[q..q+4) == a[q+4..q+8) is w[q] == w[q+4], and
        // a[q]==a[q+2] && a[q+1]==a[q+3] is w[q]'s low half == its high half
        u32 w[20];
#pragma unroll
        for (u32 j = 0; j < 5u; j++) {
          w[4u * j] = d[j];
#pragma unroll
          for (u32 k = 1; k < 4u; k++) w[4u * j + k] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], k);
        }
        m1 = ad_eq4(d[0], w[1]) | ad_eq4(d[1], w[5]) << 4 | ad_eq4(d[2], w[9]) << 8 | ad_eq4(d[3], w[13]) << 12;
#pragma unroll
        for (u32 q = 0; q < 16u; q++)
          score_full += (u32)__popcll(__ballot((w[q] & 0xFFFFu) == w[q] >> 16)) + 2u * (u32)__popcll(__ballot(w[q] == w[q + 4u]));
#pragma unroll
        for (u32 j = 0; j < 16u; j++) atomicAdd(&hw[(d[j >> 2] >> (8u * (j & 3u))) & 255u], 1u);
      } else {
        // valid bytes of the 24-byte window at W: [L, H)
        u32 const L = W >= lo ? 0u : (u32)min(lo - W, (u64)16u), H = W >= hi ? 0u : (u32)min(hi - W, (u64)24u);
        u32 const notL = ~ad_below(L);
        auto valid = [&](u32 k) { return ad_below(min(H > k ? H - k : 0u, 16u)) & notL; };  // positions q >= L with q + k < H
        m1 = ad_pair_mask(x[u], d4) & valid(1u) & (u < AD_ROWS || lane < AD_EXT ? 0xFFFFu : 0u);
        if (u < AD_ROWS) {  // (the extension only feeds the runs)
          u32 e2 = 0, e4 = 0;  // a[q] == a[q+2], a[q] == a[q+4] for q in [0, 20)
#pragma unroll
          for (u32 j = 0; j < 5u; j++) {
            e2 |= ad_eq4(d[j], __builtin_amdgcn_alignbyte(d[j + 1], d[j], 2)) << (4u * j);
            e4 |= ad_eq4(d[j], d[j + 1]) << (4u * j);
          }
          // i counts when i + 4 < n (i in [0, n-4)); the 4-byte compare when i + 8 < n
          score += __popc(e2 & e2 >> 1 & valid(4u)) + 2u * __popc(e4 & e4 >> 1 & e4 >> 2 & e4 >> 3 & valid(8u));
          u32 const v0 = valid(0u);
#pragma unroll
          for (u32 j = 0; j < 16u; j++)
            if (v0 >> j & 1u) atomicAdd(&hw[(d[j >> 2] >> (8u * (j & 3u))) & 255u], 1u);
        }
      }
      runs.row(m1, 1024u * u + 16u * lane);
      if (u < AD_ROWS) pairs += __popc(m1);
    }
    pairs = wave_sum(pairs);
    score = wave_sum(score) + score_full;
    u32 const streak = lane_value(wave_scan_max_incl(runs.best), 63u);
    if (lane == 0) {
      if (pairs) atomicAdd(&rec[ZH_AD_REC_PAIRS], pairs);
      if (score) atomicAdd(&rec[ZH_AD_REC_PATTERN], score);
      if (streak) atomicMax(&rec[ZH_AD_REC_RUN], min(streak + 1u, ZH_AD_RUN_CAP));
    }
  }
  __syncthreads();
  u32 h = 0;
#pragma unroll
  for (u32 k = 0; k < AD_SUB; k++) h += hist[AD_SUB_STRIDE * k + tid];
  if (h) atomicAdd(&rec[tid], h);
}

extern "C" __global__ __launch_bounds__(AD_THREADS) void zh_adaptive_finalize_kernel(ZhAdBatch b, const u32 *__restrict__ temp, int preference,
                                                                          cuda_zstd_adaptive_stats_t *__restrict__ stats,
                                                                          int *__restrict__ levels) {
  u32 const lane = threadIdx.x & 63u, chunk = blockIdx.x * AD_WAVES + (threadIdx.x >> 6);
  if (chunk >= b.nchunks) return;  // (whole wave; no barrier below)
  const u8 *p;
  u32 const n = ad_chunk(b, chunk, p);
  const u32 *const rec = temp + (size_t)chunk * ZH_AD_REC_WORDS;
  float const inv_n = n ? 1.0f / (float)n : 0.0f;
  float ent = 0.0f;
  u32 uniq = 0;
#pragma unroll
  for (u32 k = 0; k < 4u; k++) {
    u32 const c = rec[64u * k + lane];
    uniq += c != 0u;
    ent += zh_adaptive_entropy_term(c, inv_n);
  }
  uniq = wave_sum(uniq);
#pragma unroll
  for (u32 o = 32u; o; o >>= 1) ent += __shfl_xor(ent, (int)o);
  if (lane == 0) {
    cuda_zstd_adaptive_stats_t s;
    zh_adaptive_decide(n, rec[ZH_AD_REC_PAIRS], rec[ZH_AD_REC_RUN], rec[ZH_AD_REC_PATTERN], uniq, ent, preference, &s);
    if (stats) stats[chunk] = s;
    levels[chunk] = s.level;
  }
}

namespace zh {

uint32_t adaptive_grid(size_t num_chunks, size_t sample_bytes) {
  u64 const sample = sample_bytes < ZH_AD_MAX_SAMPLE ? (u64)sample_bytes : ZH_AD_MAX_SAMPLE;
  u64 const tiles = (sample + 15u + ZH_AD_TILE - 1u) / ZH_AD_TILE, grid = (u64)num_chunks * tiles;
  return num_chunks > 0x7FFFFFFFull || grid > 0x7FFFFFFFull ? 0u : (u32)grid;
}

hipError_t adaptive_launch(const void *const *d_ptrs, const size_t *d_sizes, const void *one_ptr, size_t one_size, size_t num_chunks,
                           size_t sample_bytes, int preference, cuda_zstd_adaptive_stats_t *d_stats, int *d_levels, uint32_t *d_temp,
                           hipStream_t stream) {
  u32 const grid = adaptive_grid(num_chunks, sample_bytes);
  if (!grid) return hipErrorInvalidValue;
  ZhAdBatch b;
  b.ptrs = d_ptrs;
  b.sizes = d_sizes;
  b.one_ptr = one_ptr;
  b.one_size = one_size;
  b.nchunks = (u32)num_chunks;
  b.tiles = grid / b.nchunks;
  b.sample = (u32)(sample_bytes < ZH_AD_MAX_SAMPLE ? sample_bytes : ZH_AD_MAX_SAMPLE);
  hipError_t const e = hipMemsetAsync(d_temp, 0, num_chunks * ZH_AD_REC_WORDS * sizeof(u32), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(zh_adaptive_analyze_kernel, dim3(grid), dim3(AD_THREADS), 0, stream, b, d_temp);
  hipLaunchKernelGGL(zh_adaptive_finalize_kernel, dim3((b.nchunks + AD_WAVES - 1u) / AD_WAVES), dim3(AD_THREADS), 0, stream, b,
                     (const u32 *)d_temp, preference, d_stats, d_levels);
  return hipGetLastError();
}

}  // namespace zh

// zh_dict_train.hip — COVER dictionary training on the device: the bytes zh::cover_train
// (zh_dict.cpp) returns, from samples that already lie in device memory.  The formulation and
// the geometry are zh_dict_plan.h's; every value is an integer, so the atomics below leave the
// result deterministic.
//
// Once per call
//   zh_cover_ids_kernel      dm[i]: hashed d-mer id of every position (NONE across a sample end)
//   zh_cover_prev_kernel     prevdist[i]: nearest earlier equal id within seg - 1 positions,
//                            a backward look over a tile of dm and its halo (in LDS while
//                            they fit in 64 KiB, from global memory for larger k)
// Once per wave of groups
//   zh_cover_freq_kernel     freq[h]: samples that contain bucket h; a workgroup walks whole
//                            samples with a 2^20-bit set in LDS and clears only the bits it set
// Once per epoch visit (the host trainer's loop body), all no-ops once the trainer is done
//   zh_cover_contrib_kernel  +f / -f of every live position into the difference array
//   zh_cover_tilesum_kernel  sum of each 2048-entry tile of it
//   zh_cover_tilescan_kernel exclusive scan of the tile sums (one workgroup)
//   zh_cover_argmax_kernel   scores = prefix sums; each tile's first maximum; clears the tile
//   zh_cover_commit_kernel   one workgroup: the epoch's first maximum, trim, zero the segment's
//                            frequencies, copy its bytes in front of the dictionary's tail
// Scores are sums of frequencies (at most num_samples * seg): the accumulators are 64-bit.
//
// One call trains one dictionary per group of consecutive samples (zh_dict_plan.h, CoverGroup);
// a single dictionary is the call with one group.  ids and prevdist run once over the whole
// concatenation (a d-mer never crosses a sample end, so one ends array gives every group's ids;
// the look-back stops at the group's first position).  The other kernels take the group from
// blockIdx.y: the groups of a wave (at most 64) share each launch, every group with its own
// CoverCtl, freq, diff, tsum, tbest and dict slot, and a workgroup past its group's samples or
// tiles, or of a group that is done, returns at once.
#include "zh_common.h"
#include "zh_dict_train.h"
#include "zh_scan.h"

#include <algorithm>

namespace {

using zh::CoverCtl;
using zh::CoverEpoch;
using zh::CoverGroup;
using zh::CoverPlan;
using zh::kCoverNone;

constexpr u32 CT = ZH_SCAN_THREADS;                      // threads of every kernel but freq
constexpr u32 FREQ_T = 1024;
constexpr u32 FREQ_WORDS = 1u << (zh::kCoverHashBits - 5);
constexpr u32 FREQ_LDS = FREQ_WORDS * 4;                 // 128 KiB
constexpr u32 PREV_TILE = 4096;                          // positions per prevdist workgroup
constexpr u32 PREV_LDS_MAX = 64 * 1024;
constexpr u32 SCAN_PER_THREAD = (u32)(zh::kCoverScanTile / CT);
static_assert(SCAN_PER_THREAD * CT == zh::kCoverScanTile, "scan tile");

struct TileBest {
  u64 score;
  u32 w;  // window start relative to the epoch's b
  u32 pad;
};
static_assert(sizeof(TileBest) == 16, "cover_temp_layout reserves 16 bytes per tile");

// the larger score, the lower w among equal scores
__device__ __forceinline__ void best_merge(u64 &s, u32 &w, u64 s2, u32 w2) {
  if (s2 > s || (s2 == s && w2 < w)) {
    s = s2;
    w = w2;
  }
}

// every thread gets the workgroup's best; lds_s / lds_w: CT / 64 entries each
__device__ __forceinline__ void block_best(u64 &s, u32 &w, u64 *lds_s, u32 *lds_w) {
  u32 const tid = threadIdx.x;
#pragma unroll
  for (u32 o = 32; o; o >>= 1) {
    u64 const s2 = __shfl_down((unsigned long long)s, o, 64);
    u32 const w2 = __shfl_down(w, o, 64);
    best_merge(s, w, s2, w2);
  }
  __syncthreads();
  if ((tid & 63u) == 0) {
    lds_s[tid >> 6] = s;
    lds_w[tid >> 6] = w;
  }
  __syncthreads();
  s = lds_s[0];
  w = lds_w[0];
#pragma unroll
  for (u32 k = 1; k < CT / 64; k++) best_merge(s, w, lds_s[k], lds_w[k]);
}

__device__ __forceinline__ u32 block_min32(u32 v, u32 *lds) {
  u32 const tid = threadIdx.x;
#pragma unroll
  for (u32 o = 32; o; o >>= 1) v = min(v, (u32)__shfl_down(v, o, 64));
  __syncthreads();
  if ((tid & 63u) == 0) lds[tid >> 6] = v;
  __syncthreads();
  u32 m = lds[0];
#pragma unroll
  for (u32 k = 1; k < CT / 64; k++) m = min(m, lds[k]);
  return m;
}

// the per-group arrays of the temp buffer: slot 0 and the byte strides of cover_temp_layout
struct Slots {
  u8 *ctl, *freq, *diff, *tsum, *tbest, *dict;
  u64 freq_stride, diff_stride, tsum_stride, tbest_stride, dict_stride;
  __host__ __device__ CoverCtl *ctl_of(u32 s) const { return (CoverCtl *)ctl + s; }
  __host__ __device__ u32 *freq_of(u32 s) const { return (u32 *)(freq + s * freq_stride); }
  __host__ __device__ u64 *diff_of(u32 s) const { return (u64 *)(diff + s * diff_stride); }
  __host__ __device__ u64 *tsum_of(u32 s) const { return (u64 *)(tsum + s * tsum_stride); }
  __host__ __device__ TileBest *tbest_of(u32 s) const { return (TileBest *)(tbest + s * tbest_stride); }
  __host__ __device__ u8 *dict_of(u32 s) const { return dict + s * dict_stride; }
};

}  // namespace

// ---------------------------------------------------------------------------------------------
// once per call
// ---------------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(256) void zh_cover_ids_kernel(const u8 *__restrict__ corpus, const u32 *__restrict__ ends, u32 ns,
                                                                      CoverPlan p, u32 *__restrict__ dm) {
  u64 const i = (u64)blockIdx.x * CT + threadIdx.x;
  if (i >= p.nd) return;
  // the sample that holds i: the first whose end lies past it (zero-size samples never do)
  u32 lo = 0, hi = ns - 1;
  while (lo < hi) {
    u32 const mid = lo + ((hi - lo) >> 1);
    if ((u64)ends[mid] <= i) lo = mid + 1;
    else hi = mid;
  }
  u32 id = kCoverNone;
  if (i + p.d <= (u64)ends[lo]) {
    const u8 *const s = corpus + i;
    u32 const sa = (u32)((uintptr_t)s & 3u);
    u64 v;
    if (i >= 4 && i + 12 <= p.N) {  // three aligned dwords inside the buffer cover s[0, 8)
      const u32 *const q = (const u32 *)(s - sa);
      u32 const a0 = q[0], a1 = q[1], a2 = sa ? q[2] : 0u;
      v = (u64)__builtin_amdgcn_alignbyte(a1, a0, sa) | (u64)__builtin_amdgcn_alignbyte(a2, a1, sa) << 32;
    } else {  // the buffer's edges: the d bytes of the d-mer only (the mask drops the others)
      v = 0;
      for (u32 j = 0; j < p.d; j++) v |= (u64)s[j] << (8 * j);
    }
    id = zh::cover_hash(v, p.mask);
  }
  dm[i] = id;
}

template <bool IN_LDS>
__global__ __launch_bounds__(256) void zh_cover_prev_kernel(const u32 *__restrict__ dm, u64 nd, u32 seg, const CoverGroup *__restrict__ groups,
                                                            u32 ng, u16 *__restrict__ prev) {
  extern __shared__ u32 win[];  // IN_LDS: dm[w0, tend)
  u32 const tid = threadIdx.x, halo = seg - 1;
  u64 const t0 = (u64)blockIdx.x * PREV_TILE, tend = min(t0 + PREV_TILE, nd);
  u64 const w0 = t0 >= halo ? t0 - halo : 0;
  const u32 *src = dm + w0;
  if (IN_LDS) {
    for (u32 j = tid; j < (u32)(tend - w0); j += CT) win[j] = dm[w0 + j];
    __syncthreads();
    src = win;
  }
  for (u64 i = t0 + tid; i < tend; i += CT) {
    u32 const c = (u32)(i - w0);  // src[c] is position i; c >= min(halo, i)
    u32 const h = src[c];
    u32 r = 0;
    if (h != kCoverNone) {
      // the group that holds i: the last whose base is not past it (groups without bytes share
      // their base with the next one, which is as good)
      u32 lo = 0, hi = ng - 1;
      while (lo < hi) {
        u32 const mid = lo + ((hi - lo + 1) >> 1);
        if (groups[mid].base <= i) lo = mid;
        else hi = mid - 1;
      }
      u32 const maxj = zh::cover_lookback(seg, i - groups[lo].base);  // <= min(halo, i)
      u32 j = 1;
      for (; j + 3 <= maxj; j += 4) {
        u32 const x0 = src[c - j], x1 = src[c - j - 1], x2 = src[c - j - 2], x3 = src[c - j - 3];
        r = x0 == h ? j : x1 == h ? j + 1 : x2 == h ? j + 2 : x3 == h ? j + 3 : 0u;
        if (r) break;
      }
      if (!r)
        for (; j <= maxj; j++)
          if (src[c - j] == h) {
            r = j;
            break;
          }
    }
    prev[i] = (u16)r;
  }
}

// ---------------------------------------------------------------------------------------------
// once per wave of groups: blockIdx.y is the group of the wave
// ---------------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(1024) void zh_cover_freq_kernel(const CoverGroup *__restrict__ groups, Slots S,
                                                                        const u32 *__restrict__ dm, const u32 *__restrict__ ends) {
  extern __shared__ u32 bits[];  // FREQ_WORDS: the buckets seen in the current sample
  CoverGroup const &g = groups[blockIdx.y];
  // = g.slot, as a wave starts at a multiple of the slot count: the slot's addresses do not wait for the load of g
  u32 const slot = blockIdx.y;
  if (g.plan.empty || g.s0 + blockIdx.x >= g.s1) return;
  u32 const tid = threadIdx.x;
  u32 *const freq = S.freq_of(slot);
  u64 const gend = g.base + g.plan.nd;  // the group's last d-mer starts before it
  for (u32 k = tid; k < FREQ_WORDS; k += FREQ_T) bits[k] = 0;
  __syncthreads();
  for (u32 s = g.s0 + blockIdx.x; s < g.s1; s += gridDim.x) {
    u64 const a = s ? ends[s - 1] : 0u, e = min((u64)ends[s], gend);
    for (u64 i = a + tid; i < e; i += FREQ_T) {
      u32 const h = dm[i];
      if (h == kCoverNone) continue;
      u32 const m = 1u << (h & 31u);
      if (!(atomicOr(&bits[h >> 5], m) & m)) atomicAdd(&freq[h], 1u);
    }
    __syncthreads();
    for (u64 i = a + tid; i < e; i += FREQ_T) {  // every set bit of a word is this sample's
      u32 const h = dm[i];
      if (h != kCoverNone) bits[h >> 5] = 0;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// one epoch visit of every group of the wave: positions, windows and tiles are group-local, the
// loads of dm, prev and the corpus add the group's base
// ---------------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(256) void zh_cover_contrib_kernel(const CoverGroup *__restrict__ groups, Slots S,
                                                                          const u32 *__restrict__ dm, const u16 *__restrict__ prev) {
  CoverGroup const &g = groups[blockIdx.y];
  u32 const slot = blockIdx.y;  // = g.slot
  const CoverCtl *const ctl = S.ctl_of(slot);
  if (ctl->done) return;
  CoverEpoch const ep = zh::cover_epoch(g.plan, ctl->epoch);
  u64 const i = ep.b + (u64)blockIdx.x * CT + threadIdx.x;
  if (i >= ep.end) return;
  u32 const h = dm[g.base + i];
  if (h == kCoverNone) return;
  u64 const f = S.freq_of(slot)[h];
  if (!f) return;
  size_t lo, hi;
  if (!zh::cover_range(i, prev[g.base + i], g.plan.seg, ep, lo, hi)) return;
  // lo - b <= hi + 1 - b <= wmax + 1 - b <= esz: inside the group's ntiles * 2048 entries of diff
  u64 *const diff = S.diff_of(slot);
  atomicAdd((unsigned long long *)&diff[lo - ep.b], (unsigned long long)f);
  atomicAdd((unsigned long long *)&diff[hi + 1 - ep.b], (unsigned long long)(0ull - f));
}

extern "C" __global__ __launch_bounds__(256) void zh_cover_tilesum_kernel(const CoverGroup *__restrict__ groups, Slots S) {
  __shared__ u64 lds[CT / 64];
  CoverGroup const &g = groups[blockIdx.y];
  u32 const slot = blockIdx.y;  // = g.slot
  if (blockIdx.x >= g.ntiles || S.ctl_of(slot)->done) return;
  const u64 *const q = S.diff_of(slot) + (size_t)blockIdx.x * zh::kCoverScanTile + (size_t)threadIdx.x * SCAN_PER_THREAD;
  u64 s = 0;
#pragma unroll
  for (u32 j = 0; j < SCAN_PER_THREAD; j++) s += q[j];
  u64 total;
  (void)block_scan_excl64(s, lds, total);
  if (threadIdx.x == 0) S.tsum_of(slot)[blockIdx.x] = total;
}

extern "C" __global__ __launch_bounds__(256) void zh_cover_tilescan_kernel(const CoverGroup *__restrict__ groups, Slots S) {
  __shared__ u64 lds[CT / 64];
  CoverGroup const &g = groups[blockIdx.y];
  u32 const slot = blockIdx.y;  // = g.slot
  if (S.ctl_of(slot)->done) return;
  u64 *const tsum = S.tsum_of(slot);
  u32 const ntiles = g.ntiles;
  u64 carry = 0;
  for (u32 t0 = 0; t0 < ntiles; t0 += CT) {
    u32 const t = t0 + threadIdx.x;
    u64 const v = t < ntiles ? tsum[t] : 0ull;
    u64 total;
    u64 const ex = block_scan_excl64(v, lds, total);
    if (t < ntiles) tsum[t] = carry + ex;
    carry += total;
  }
}

extern "C" __global__ __launch_bounds__(256) void zh_cover_argmax_kernel(const CoverGroup *__restrict__ groups, Slots S) {
  __shared__ u64 lds[CT / 64];
  __shared__ u32 ldw[CT / 64];
  CoverGroup const &g = groups[blockIdx.y];
  u32 const slot = blockIdx.y;  // = g.slot
  const CoverCtl *const ctl = S.ctl_of(slot);
  if (blockIdx.x >= g.ntiles || ctl->done) return;
  CoverEpoch const ep = zh::cover_epoch(g.plan, ctl->epoch);
  u64 const nw = ep.wmax - ep.b + 1;
  u64 const i0 = (u64)blockIdx.x * zh::kCoverScanTile + (u64)threadIdx.x * SCAN_PER_THREAD;
  u64 *const q = S.diff_of(slot) + i0;
  u64 v[SCAN_PER_THREAD], s = 0;
#pragma unroll
  for (u32 j = 0; j < SCAN_PER_THREAD; j++) {
    v[j] = q[j];
    q[j] = 0;  // the next step starts from a clear array
    s += v[j];
  }
  u64 total;
  u64 run = S.tsum_of(slot)[blockIdx.x] + block_scan_excl64(s, lds, total);
  u64 best = 0;
  u32 bw = ~0u;
#pragma unroll
  for (u32 j = 0; j < SCAN_PER_THREAD; j++) {
    run += v[j];
    if (i0 + j < nw && run > best) {  // strict: the first maximum
      best = run;
      bw = (u32)(i0 + j);
    }
  }
  block_best(best, bw, lds, ldw);
  if (threadIdx.x == 0) {
    TileBest b;
    b.score = best;
    b.w = bw;
    b.pad = 0;
    S.tbest_of(slot)[blockIdx.x] = b;
  }
}

extern "C" __global__ __launch_bounds__(256) void zh_cover_commit_kernel(const CoverGroup *__restrict__ groups, Slots S,
                                                                         const u32 *__restrict__ dm, const u8 *__restrict__ corpus) {
  __shared__ u64 lds[CT / 64];
  __shared__ u32 ldw[CT / 64];
  u32 const tid = threadIdx.x;
  CoverGroup const &g = groups[blockIdx.y];
  u32 const slot = blockIdx.y;  // = g.slot
  CoverCtl *const ctl = S.ctl_of(slot);
  if (ctl->done) return;
  CoverPlan const &p = g.plan;
  const TileBest *const tbest = S.tbest_of(slot);
  u32 *const freq = S.freq_of(slot);
  const u32 *const gdm = dm + g.base;  // the group's ids and bytes, by group-local position
  const u8 *const gcorpus = corpus + g.base;
  u32 const e = ctl->epoch, tail = ctl->tail, zero_run = ctl->zero_run;
  CoverEpoch const ep = zh::cover_epoch(p, e);
  u64 best = 0;
  u32 bw = ~0u;
  for (u32 t = tid; t < g.ntiles; t += CT) best_merge(best, bw, tbest[t].score, tbest[t].w);
  block_best(best, bw, lds, ldw);  // (its barriers also order the reads of ctl above before the writes below)
  u32 const next = (u32)((e + 1) % p.epochs);
  if (best == 0) {
    if (tid == 0) {
      ctl->zero_run = zero_run + 1;
      if (zero_run + 1 >= p.max_zero) ctl->done = 1;
      ctl->epoch = next;
    }
    return;
  }
  // trim the segment over positions that score nothing, by freq as it is before zeroing
  u64 const sb0 = ep.b + bw, se0 = min((u64)ep.end, sb0 + p.seg);
  u32 const len = (u32)(se0 - sb0);
  u32 first = len, last1 = 0;  // first live offset; 1 + the last live offset (max as min of the complement)
  for (u32 o = tid; o < len; o += CT) {
    u32 const h = gdm[sb0 + o];
    if (h != kCoverNone && freq[h] != 0) {
      first = min(first, o);
      last1 = max(last1, o + 1);
    }
  }
  first = block_min32(first, ldw);
  last1 = ~block_min32(~last1, ldw);
  u64 const sb = sb0 + first, se = last1 > first ? sb0 + last1 : sb;  // (none live: empty, as the host's loops leave it)
  __syncthreads();  // every read of freq is done
  for (u64 i = sb + tid; i < se; i += CT) {
    u32 const h = gdm[i];
    if (h != kCoverNone) freq[h] = 0;
  }
  size_t const bytes = zh::cover_commit_bytes(sb, se, p.d, tail);
  if (bytes < p.d) {
    if (tid == 0) ctl->done = 1;
    return;
  }
  u32 const ntail = tail - (u32)bytes;
  // sb + bytes <= se + d - 1 <= nd + d - 1 = N of the group; ntail + bytes = tail <= dict_size
  u8 *const dict = S.dict_of(slot);
  for (u32 o = tid; o < (u32)bytes; o += CT) dict[ntail + o] = gcorpus[sb + o];
  if (tid == 0) {
    ctl->tail = ntail;
    ctl->zero_run = 0;
    if (ntail == 0) ctl->done = 1;
    ctl->epoch = next;
  }
}

namespace zh {

hipError_t cover_train_groups_device(const uint8_t *d_corpus, const uint32_t *ends, size_t ns, const CoverGroup *groups, size_t ng,
                                     size_t dict_size, void *temp, hipStream_t stream, std::vector<std::vector<uint8_t>> &out, float *phase_ms) {
  out.assign(ng, std::vector<uint8_t>());
  if (phase_ms) phase_ms[0] = phase_ms[1] = phase_ms[2] = 0.f;
  if (!d_corpus || !ends || !ns || !groups || !ng || ng > kCoverMaxGroups || !temp || ns >= (1ull << 32) || dict_size >= (1ull << 32))
    return hipErrorInvalidValue;
  u64 const N = groups[ng - 1].base + groups[ng - 1].plan.N;
  if (N >= (1ull << 32) - 64 || groups[0].plan.k > kCoverMaxK || groups[ng - 1].s1 != ns) return hipErrorInvalidValue;
  size_t max_ntiles = 0;
  bool any = false;
  for (size_t g = 0; g < ng; g++) {
    max_ntiles = std::max<size_t>(max_ntiles, groups[g].ntiles);
    any = any || !groups[g].plan.empty;
  }
  if (!any) return hipSuccess;  // every group has fewer than k bytes: the host trainer's empty results
  // ids and prevdist of the whole concatenation: k, d, the mask and seg are the same in every plan
  CoverPlan const whole = cover_plan((size_t)N, dict_size, groups[0].plan.k, groups[0].plan.d);
  // (per device, so set on every call; it costs no launch)
  hipError_t const ia = hipFuncSetAttribute((const void *)zh_cover_freq_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FREQ_LDS);
  if (ia != hipSuccess) return ia;
  int dev = 0, cus = 0;
  if (stream) (void)hipStreamGetDevice(stream, &dev);
  else (void)hipGetDevice(&dev);
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;

  CoverTempLayout const L = cover_temp_layout((size_t)N, ns, ng, max_ntiles, dict_size);
  u8 *const base = (u8 *)(((uintptr_t)temp + 255) & ~(uintptr_t)255);
  CoverGroup *const d_groups = (CoverGroup *)(base + L.groups);
  u32 *const d_ends = (u32 *)(base + L.ends), *const dm = (u32 *)(base + L.dm);
  u16 *const prev = (u16 *)(base + L.prev);
  Slots S;
  S.ctl = base + L.ctl, S.freq = base + L.freq, S.diff = base + L.diff, S.tsum = base + L.tsum, S.tbest = base + L.tbest, S.dict = base + L.dict;
  S.freq_stride = L.freq_stride, S.diff_stride = L.diff_stride, S.tsum_stride = L.tsum_stride, S.tbest_stride = L.tbest_stride;
  S.dict_stride = L.dict_stride;

  // the host sides of every copy below live until the function's last synchronisation
  std::vector<CoverCtl> ctl0(ng), h_ctl(L.slots);
  for (size_t g = 0; g < ng; g++) ctl0[g] = CoverCtl{(u32)dict_size, 0u, 0u, groups[g].plan.empty ? 1u : 0u};
  std::vector<u8> h_dict(L.slots * L.dict_stride);

  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // call: 0 ids 1 prev 2; wave: 3 freq 4 steps 5
  hipError_t err = hipSuccess;
  auto ok = [&](hipError_t e) {
    if (err == hipSuccess && e != hipSuccess) err = e;
    return err == hipSuccess;
  };
  auto mark = [&](int k) {
    if (phase_ms && err == hipSuccess) ok(hipEventRecord(ev[k], stream));
  };
  auto add = [&](int phase, int k) {  // after a synchronisation
    float ms = 0.f;
    if (phase_ms && ok(hipEventElapsedTime(&ms, ev[k], ev[k + 1]))) phase_ms[phase] += ms;
  };
  if (phase_ms)
    for (auto &e : ev) ok(hipEventCreate(&e));

  ok(hipMemcpyAsync(d_groups, groups, ng * sizeof(CoverGroup), hipMemcpyHostToDevice, stream)) &&
      ok(hipMemcpyAsync(d_ends, ends, ns * 4, hipMemcpyHostToDevice, stream));
  mark(0);
  if (err == hipSuccess) {
    hipLaunchKernelGGL(zh_cover_ids_kernel, dim3((u32)((whole.nd + CT - 1) / CT)), dim3(CT), 0, stream, d_corpus, d_ends, (u32)ns, whole, dm);
    ok(hipGetLastError());
  }
  mark(1);
  if (err == hipSuccess) {
    u32 const grid = (u32)((whole.nd + PREV_TILE - 1) / PREV_TILE);
    size_t const lds = (PREV_TILE + whole.seg - 1) * 4;
    if (lds <= PREV_LDS_MAX)
      hipLaunchKernelGGL(zh_cover_prev_kernel<true>, dim3(grid), dim3(CT), (u32)lds, stream, dm, (u64)whole.nd, (u32)whole.seg, d_groups, (u32)ng,
                         prev);
    else
      hipLaunchKernelGGL(zh_cover_prev_kernel<false>, dim3(grid), dim3(CT), 0, stream, dm, (u64)whole.nd, (u32)whole.seg, d_groups, (u32)ng, prev);
    ok(hipGetLastError());
  }
  mark(2);

  bool first_wave = true;
  for (size_t g0 = 0; g0 < ng && err == hipSuccess; g0 += kCoverGroupsInFlight) {
    u32 const gn = (u32)std::min<size_t>(kCoverGroupsInFlight, ng - g0);
    // what the launches of this wave must cover: its live groups' samples, epochs, positions and tiles
    size_t samples = 0, epochs = 0, esz = 0, ntiles = 0;
    for (u32 j = 0; j < gn; j++) {
      CoverGroup const &G = groups[g0 + j];
      if (G.plan.empty) continue;
      samples = std::max<size_t>(samples, G.s1 - G.s0);
      epochs = std::max(epochs, G.plan.epochs);
      esz = std::max(esz, G.plan.esz);
      ntiles = std::max<size_t>(ntiles, G.ntiles);
    }
    if (!samples) continue;  // no live group
    const CoverGroup *const wg = d_groups + g0;
    ok(hipMemcpyAsync(S.ctl, &ctl0[g0], gn * sizeof(CoverCtl), hipMemcpyHostToDevice, stream)) &&
        ok(hipMemsetAsync(S.freq, 0, gn * L.freq_stride, stream)) && ok(hipMemsetAsync(S.diff, 0, gn * L.diff_stride, stream));
    mark(3);
    if (err == hipSuccess) {
      // about one workgroup per CU over the wave (each holds 128 KiB of LDS), at most one per sample
      u32 const bx = (u32)std::min<size_t>(samples, std::max<size_t>(1, ((size_t)cus + gn - 1) / gn));
      hipLaunchKernelGGL(zh_cover_freq_kernel, dim3(bx, gn), dim3(FREQ_T), FREQ_LDS, stream, wg, S, dm, d_ends);
      ok(hipGetLastError());
    }
    mark(4);
    // The control words come back once per pass over the epochs (at most 64 steps, so a corpus of
    // many epochs does not queue thousands of no-op steps behind dictionaries that are already
    // full).  Every step of a group that is not a no-op shrinks its tail or grows its zero_run,
    // so the loop ends.
    size_t const pass = std::min<size_t>(epochs, 64);
    u32 const cgrid = (u32)((esz + CT - 1) / CT), nt = (u32)ntiles;
    bool done = false;
    while (err == hipSuccess && !done) {
      for (size_t s = 0; s < pass; s++) {
        hipLaunchKernelGGL(zh_cover_contrib_kernel, dim3(cgrid, gn), dim3(CT), 0, stream, wg, S, dm, prev);
        hipLaunchKernelGGL(zh_cover_tilesum_kernel, dim3(nt, gn), dim3(CT), 0, stream, wg, S);
        hipLaunchKernelGGL(zh_cover_tilescan_kernel, dim3(1, gn), dim3(CT), 0, stream, wg, S);
        hipLaunchKernelGGL(zh_cover_argmax_kernel, dim3(nt, gn), dim3(CT), 0, stream, wg, S);
        hipLaunchKernelGGL(zh_cover_commit_kernel, dim3(1, gn), dim3(CT), 0, stream, wg, S, dm, d_corpus);
      }
      ok(hipGetLastError()) && ok(hipMemcpyAsync(h_ctl.data(), S.ctl, gn * sizeof(CoverCtl), hipMemcpyDeviceToHost, stream)) &&
          ok(hipStreamSynchronize(stream));
      done = true;
      for (u32 j = 0; j < gn; j++) done = done && h_ctl[j].done;
    }
    mark(5);
    ok(hipMemcpyAsync(h_dict.data(), S.dict, gn * L.dict_stride, hipMemcpyDeviceToHost, stream)) && ok(hipStreamSynchronize(stream));
    if (err != hipSuccess) break;
    for (u32 j = 0; j < gn; j++) {
      if (groups[g0 + j].plan.empty || h_ctl[j].tail > dict_size) continue;
      const u8 *const d = h_dict.data() + j * L.dict_stride;
      out[g0 + j].assign(d + h_ctl[j].tail, d + dict_size);
    }
    if (first_wave) add(0, 0), add(1, 1);
    first_wave = false;
    add(0, 3), add(2, 4);
  }
  // the host sources of the copies above stay alive until the stream has drained, errors included
  (void)hipStreamSynchronize(stream);
  for (auto &e : ev)
    if (e) (void)hipEventDestroy(e);
  if (err != hipSuccess) out.assign(ng, std::vector<uint8_t>());
  return err;
}

}  // namespace zh


// zh_frames.hip — the seek table of concatenated Zstandard frames that carry none (one frame's
// extent: zh_frames.h; the table's format: zh_seek_format.h).
//
// Finding the frames one after another is a chain of dependent loads, two or more per frame.  The
// speculative index breaks the chain: every position that could start a frame is found at memory
// bandwidth, each candidate's frame is walked independently, and the candidates that the walk from
// offset 0 really visits are selected by pointer doubling.  No workgroup waits on another.
//   zh_frames_count_kernel  : per 4 KiB tile, the positions whose u32 is a frame magic or one of
//                             the 16 skippable magics (offset 0 always counts)
//   zh_frames_sums_kernel   : one workgroup scans the tile counts into tile bases
//   zh_frames_write_kernel  : the candidates' offsets, compacted in ascending order
//   zh_frames_span_kernel   : one lane per candidate: zh_frame_span, then the candidate at the
//                             frame's end by binary search (its `next`).  Two absorbing nodes close
//                             the graph: END (the frame ends with the stream) and BAD (malformed,
//                             or the end is inside the stream and no candidate)
//   zh_frames_reach_kernel  : round k of the doubling: every marked node marks jump_k[c] with
//                             rank[c] + 2^k (the minimum wins), and jump_{k+1} = jump_k o jump_k
//   zh_frames_collect_kernel: one lane per marked candidate: entry `rank`, a size job for a frame
//                             without a Frame_Content_Size, and the stream's verdict
//   zh_frames_walk_kernel   : the serial walker -- the same outputs frame after frame (more
//                             candidates than the temp buffer holds, or the test hook)
//   zh_frames_sizes_kernel  : after the decoder's size pass over the jobs: sizes into entries
//   zh_frames_emit_kernel   : the table.  Nothing of it is written before the call has succeeded.
#include "zh_frames_index.h"
#include "zh_scan.h"

#include <algorithm>

namespace {

constexpr u32 FR_THREADS = ZH_SCAN_THREADS;
constexpr u32 FR_INF = 0xFFFFFFFFu;
constexpr u64 FR_NONE = ~0ull;
static_assert(FR_THREADS * ZH_FRAMES_LANE_BYTES == ZH_FRAMES_TILE, "zh_frames.h states the tile");

__host__ __device__ inline size_t fr_align256(size_t v) { return (v + 255) & ~(size_t)255; }
// tiles of a stream whose pointer has the low bits a (< 16)
__host__ __device__ inline u64 fr_tiles(u64 size, u64 a) { return (a + size + ZH_FRAMES_TILE - 1) / ZH_FRAMES_TILE; }

struct FramesLayout {
  size_t ctl, tiles, cand, fsize, ffcs, info, next, jump_a, jump_b, rank, entry_c, entry_d, in_ptrs, in_sizes, out_sizes, statuses,
      job_entry, total;
  static FramesLayout make(size_t stream_bytes, size_t n) {
    FramesLayout L{};
    size_t const nt = (size_t)fr_tiles(stream_bytes, 15), c = (size_t)ZH_FRAMES_CANDIDATES(n);
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t const at = o; o = fr_align256(o + bytes); return at; };
    L.ctl = take(sizeof(zh::FramesCtl));
    L.tiles = take(nt * 4);
    L.cand = take(c * 8);
    L.fsize = take(c * 8);
    L.ffcs = take(c * 8);
    L.info = take(c * 4);
    L.next = take((c + 2) * 4);
    L.jump_a = take((c + 2) * 4);
    L.jump_b = take((c + 2) * 4);
    L.rank = take((c + 2) * 4);
    L.entry_c = take(n * 4);
    L.entry_d = take(n * 4);
    L.in_ptrs = take(n * 8);
    L.in_sizes = take(n * 8);
    L.out_sizes = take(n * 8);
    L.statuses = take(n * 4);
    L.job_entry = take(n * 4);
    L.total = o + 256;  // slack for base alignment
    return L;
  }
};

// What the walk leaves for the later kernels: the entries' two columns and the size jobs
struct FramesOut {
  u32 *entry_c, *entry_d;
  const void **in_ptrs;
  size_t *in_sizes;
  u32 *job_entry;
  u64 max_frames;
};

__device__ __forceinline__ u32 block_scan_excl32(u32 v, u32 *lds, u32 &total) {
  u32 const tid = threadIdx.x, w = tid >> 6;
  u32 const inc = wave_scan_incl(v);
  __syncthreads();
  if ((tid & 63u) == 63u) lds[w] = inc;
  __syncthreads();
  u32 base = 0, tot = 0;
#pragma unroll
  for (u32 k = 0; k < FR_THREADS / 64; k++) {
    u32 const s = lds[k];
    base += k < w ? s : 0u;
    tot += s;
  }
  total = tot;
  return base + inc - v;
}

// The candidates among the 16 positions v0 .. v0 + 15 (bit j: position v0 + j), in the coordinates
// of the 16-byte-aligned pointer b = stream - a: offset = v - a.  A position counts when its four
// bytes lie inside the stream and spell a magic; offset 0 always counts.  Loads: the aligned 16
// bytes at v0 and the dword behind them, each only when it holds a byte of the stream.
__device__ __forceinline__ u32 lane_candidates(const u8 *b, u64 a, u64 size, u64 v0) {
  u64 const vend = a + size;
  if (v0 >= vend) return 0;  // (v0 + 16 > a always: a < 16)
  uint4 const q = *(const uint4 *)(b + v0);
  u32 const w[5] = {q.x, q.y, q.z, q.w, v0 + 16 < vend ? *(const u32 *)(b + v0 + 16) : 0u};
  u32 m = 0;
#pragma unroll
  for (u32 j = 0; j < 16; j++) {
    u32 const x = __builtin_amdgcn_alignbyte(w[j / 4 + 1], w[j / 4], j & 3u);
    if (zh_frames_is_magic(x)) m |= 1u << j;
  }
  u32 const lo = v0 < a ? (u32)(a - v0) : 0u;                                   // positions before the stream
  u32 const hi = v0 + 19 <= vend ? 16u : vend >= v0 + 4 ? (u32)(vend - 3 - v0) : 0u;  // positions with four bytes
  m &= (hi >= 16 ? 0xFFFFu : (1u << hi) - 1u) & ~((1u << lo) - 1u);
  if (v0 <= a) m |= 1u << (u32)(a - v0);
  return m;
}

// One complete frame of the walk, entry r: its columns, or its size job.  Entries past max_frames
// are counted by the caller and not stored.
__device__ __forceinline__ void note_frame(const u8 *stream, u64 off, u64 fsize, u64 fcs, u32 skippable, u64 r, zh::FramesCtl *ctl,
                                           const FramesOut &o) {
  if (r >= o.max_frames) return;
  u64 d = skippable ? 0ull : fcs;
  bool over = !zh_seek_field_ok(fsize);
  if (!skippable && fcs == ZH_FRAMES_NO_FCS) {
    u32 const j = atomicAdd(&ctl->njobs, 1u);
    o.in_ptrs[j] = stream + off;
    o.in_sizes[j] = (size_t)fsize;
    o.job_entry[j] = (u32)r;
    d = 0;
  } else if (!zh_seek_field_ok(d)) {
    over = true;
  }
  if (over) atomicOr(&ctl->limit, 1u);
  o.entry_c[r] = over ? 0u : (u32)fsize;
  o.entry_d[r] = over ? 0u : (u32)d;
}

}  // namespace

extern "C" __global__ __launch_bounds__(256) void zh_frames_count_kernel(const u8 *__restrict__ stream, u64 size, u32 ntiles,
                                                                         u32 *__restrict__ tcount) {
  __shared__ u32 lds[4];
  u64 const a = (uintptr_t)stream & 15u;
  const u8 *const b = stream - a;
  for (u32 t = blockIdx.x; t < ntiles; t += gridDim.x) {
    u32 const m = lane_candidates(b, a, size, (u64)t * ZH_FRAMES_TILE + threadIdx.x * ZH_FRAMES_LANE_BYTES);
    u32 total;
    (void)block_scan_excl32(__popc(m), lds, total);
    if (threadIdx.x == 0) tcount[t] = total;
  }
}

// In place: counts become exclusive bases (kept only while they fit the capacity, which is below 2^32)
extern "C" __global__ __launch_bounds__(256) void zh_frames_sums_kernel(u32 *__restrict__ tiles, u32 ntiles, zh::FramesCtl *ctl) {
  __shared__ u64 lds[4];
  u32 const tid = threadIdx.x;
  u64 carry = 0;
  for (u32 c0 = 0; c0 < ntiles; c0 += FR_THREADS) {
    u32 const t = c0 + tid;
    u64 const v = t < ntiles ? tiles[t] : 0ull;
    u64 total;
    u64 const ex = block_scan_excl64(v, lds, total);
    if (t < ntiles) tiles[t] = (u32)min(carry + ex, (u64)FR_INF);
    carry += total;
  }
  if (tid == 0) ctl->ncand = carry;
}

// ncand <= the capacity of cand[] (the host launches this only then)
extern "C" __global__ __launch_bounds__(256) void zh_frames_write_kernel(const u8 *__restrict__ stream, u64 size, u32 ntiles,
                                                                         const u32 *__restrict__ tbase, u64 ncand, u64 *__restrict__ cand) {
  __shared__ u32 lds[4];
  u64 const a = (uintptr_t)stream & 15u;
  const u8 *const b = stream - a;
  for (u32 t = blockIdx.x; t < ntiles; t += gridDim.x) {
    u64 const v0 = (u64)t * ZH_FRAMES_TILE + threadIdx.x * ZH_FRAMES_LANE_BYTES;
    u32 m = lane_candidates(b, a, size, v0);
    u32 total;
    u64 at = (u64)tbase[t] + block_scan_excl32(__popc(m), lds, total);
    while (m) {
      u32 const j = (u32)__ffs((int)m) - 1u;
      m &= m - 1u;
      if (at < ncand) cand[at] = v0 + j - a;
      at++;
    }
  }
}

// Nodes: candidates 0 .. nc - 1, END = nc, BAD = nc + 1
extern "C" __global__ __launch_bounds__(256) void zh_frames_span_kernel(const u8 *__restrict__ stream, u64 size, u32 nc,
                                                                        const u64 *__restrict__ cand, u64 *__restrict__ fsize,
                                                                        u64 *__restrict__ ffcs, u32 *__restrict__ info, u32 *__restrict__ next,
                                                                        u32 *__restrict__ jump, u32 *__restrict__ rank) {
  u32 const end_node = nc, bad_node = nc + 1;
  for (u64 c = (u64)blockIdx.x * FR_THREADS + threadIdx.x; c < (u64)nc + 2; c += (u64)gridDim.x * FR_THREADS) {
    u32 nx = (u32)c;  // the absorbing nodes point at themselves
    if (c < nc) {
      u64 const off = cand[c];
      ZhFrameSpan s{};
      u32 const st = zh_frame_span(stream + off, size - off, c == 0, &s);
      nx = bad_node;
      if (st == ZH_FRAMES_OK) {
        u64 const e = off + s.size;
        if (e == size) {
          nx = end_node;
        } else {  // (e < size) the first candidate at or after e
          u32 lo = (u32)c + 1, hi = nc;
          while (lo < hi) {
            u32 const mid = lo + (hi - lo) / 2;
            if (cand[mid] < e) lo = mid + 1;
            else hi = mid;
          }
          if (lo < nc && cand[lo] == e) nx = lo;
        }
      }
      fsize[c] = s.size;
      ffcs[c] = s.fcs;
      info[c] = st << 8 | s.skippable;
      next[c] = nx;
    }
    jump[c] = nx;
    rank[c] = c == 0 ? 0u : FR_INF;
  }
}

// A marked node's rank is its distance from candidate 0: only nodes on that one path are ever
// marked, and an absorbing node keeps the smallest rank that reaches it.
extern "C" __global__ __launch_bounds__(256) void zh_frames_reach_kernel(u32 nc, u32 k, const u32 *__restrict__ jin, u32 *__restrict__ jout,
                                                                         u32 *rank) {
  for (u64 c = (u64)blockIdx.x * FR_THREADS + threadIdx.x; c < (u64)nc + 2; c += (u64)gridDim.x * FR_THREADS) {
    u32 const j = jin[c];
    u32 const r = c < nc ? __hip_atomic_load(&rank[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : FR_INF;
    if (r != FR_INF) atomicMin(&rank[j], r + (1u << k));
    jout[c] = jin[j];
  }
}

extern "C" __global__ __launch_bounds__(256) void zh_frames_collect_kernel(const u8 *__restrict__ stream, u32 nc, const u64 *__restrict__ cand,
                                                                           const u64 *__restrict__ fsize, const u64 *__restrict__ ffcs,
                                                                           const u32 *__restrict__ info, const u32 *__restrict__ next,
                                                                           const u32 *__restrict__ rank, zh::FramesCtl *ctl, FramesOut o) {
  u32 const end_node = nc, bad_node = nc + 1;
  for (u64 c = (u64)blockIdx.x * FR_THREADS + threadIdx.x; c < nc; c += (u64)gridDim.x * FR_THREADS) {
    u32 const r = rank[c];
    if (r == FR_INF) continue;
    u32 const st = info[c] >> 8, nx = next[c];
    u64 const off = cand[c];
    if (st == ZH_FRAMES_OK) note_frame(stream, off, fsize[c], ffcs[c], info[c] & 1u, r, ctl, o);
    if (nx == end_node) {
      ctl->nframes = (u64)r + 1;
    } else if (nx == bad_node) {  // the one marked node in front of BAD: this frame fails, or the bytes at its end do
      ctl->status = st != ZH_FRAMES_OK ? st : (u32)ZH_FRAMES_CORRUPT;
      ctl->nframes = st != ZH_FRAMES_OK ? (u64)r : (u64)r + 1;
      ctl->err_off = st != ZH_FRAMES_OK ? off : off + fsize[c];
    }
  }
}

extern "C" __global__ __launch_bounds__(64) void zh_frames_walk_kernel(const u8 *__restrict__ stream, u64 size, zh::FramesCtl *ctl, FramesOut o) {
  if (threadIdx.x != 0) return;
  u64 ip = 0, nf = 0;
  u32 st = ZH_FRAMES_OK;
  while (ip < size) {
    ZhFrameSpan s{};
    st = zh_frame_span(stream + ip, size - ip, ip == 0, &s);
    if (st != ZH_FRAMES_OK) break;
    note_frame(stream, ip, s.size, s.fcs, s.skippable, nf, ctl, o);
    ip += s.size;
    nf++;
  }
  ctl->status = st;
  ctl->nframes = nf;
  ctl->err_off = st != ZH_FRAMES_OK ? ip : 0ull;
}

extern "C" __global__ __launch_bounds__(256) void zh_frames_sizes_kernel(const u8 *__restrict__ stream, u32 njobs, const void *const *__restrict__ in_ptrs,
                                                                         const size_t *__restrict__ out_sizes, const int *__restrict__ statuses,
                                                                         const u32 *__restrict__ job_entry, u32 *__restrict__ entry_d,
                                                                         zh::FramesCtl *ctl) {
  for (u64 j = (u64)blockIdx.x * FR_THREADS + threadIdx.x; j < njobs; j += (u64)gridDim.x * FR_THREADS) {
    u32 const e = job_entry[j];
    u32 code = (u32)statuses[j];
    if (code) {
      code = (code & 0xFFu) ? (code & 0xFFu) : 1u;
      // (a later entry starts at a larger offset: both minima are the same job's)
      atomicMin((unsigned long long *)&ctl->errkey, (unsigned long long)((u64)e << 8 | code));
      atomicMin((unsigned long long *)&ctl->job_err_off, (unsigned long long)((const u8 *)in_ptrs[j] - stream));
    } else if (!zh_seek_field_ok(out_sizes[j])) {
      atomicOr(&ctl->limit, 1u);
    } else {
      entry_d[e] = (u32)out_sizes[j];
    }
  }
}

extern "C" __global__ __launch_bounds__(256) void zh_frames_emit_kernel(u64 n, const u32 *__restrict__ entry_c, const u32 *__restrict__ entry_d,
                                                                        u8 *table) {
  for (u64 i = (u64)blockIdx.x * FR_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * FR_THREADS)
    zh_seek_write_entry(table + 8 + i * 8, entry_c[i], entry_d[i], 0, 0);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    zh_seek_write_header(table, n, 0);
    zh_seek_write_footer(table + 8 + n * 8, n, 0);
  }
}

// ---------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------
namespace zh {

namespace {
constexpr u32 FR_GRID_MAX = 4096;  // more work strides the grid
u32 fr_grid(u64 items) { return (u32)std::min<u64>(std::max<u64>((items + FR_THREADS - 1) / FR_THREADS, 1), FR_GRID_MAX); }

FramesOut frames_out(u8 *base, const FramesLayout &L, size_t max_frames) {
  FramesOut o;
  o.entry_c = (u32 *)(base + L.entry_c);
  o.entry_d = (u32 *)(base + L.entry_d);
  o.in_ptrs = (const void **)(base + L.in_ptrs);
  o.in_sizes = (size_t *)(base + L.in_sizes);
  o.job_entry = (u32 *)(base + L.job_entry);
  o.max_frames = max_frames;
  return o;
}
}  // namespace

size_t frames_temp_bytes(size_t stream_bytes, size_t max_frames) { return FramesLayout::make(stream_bytes, max_frames).total; }

FramesJobs frames_jobs(u8 *base, size_t stream_bytes, size_t max_frames) {
  FramesLayout const L = FramesLayout::make(stream_bytes, max_frames);
  FramesJobs j;
  j.in_ptrs = (const void **)(base + L.in_ptrs);
  j.in_sizes = (size_t *)(base + L.in_sizes);
  j.out_sizes = (size_t *)(base + L.out_sizes);
  j.statuses = (int *)(base + L.statuses);
  return j;
}

hipError_t frames_count_launch(const void *d_stream, size_t size, size_t max_frames, u8 *base, hipStream_t stream) {
  FramesLayout const L = FramesLayout::make(size, max_frames);
  FramesCtl *const ctl = (FramesCtl *)(base + L.ctl);
  hipError_t e = hipMemsetAsync(ctl, 0, sizeof(FramesCtl), stream);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(&ctl->errkey, 0xFF, 16, stream)) != hipSuccess) return e;  // errkey, job_err_off: none
  u32 const nt = (u32)fr_tiles(size, (uintptr_t)d_stream & 15u);
  u32 *const tiles = (u32 *)(base + L.tiles);
  hipLaunchKernelGGL(zh_frames_count_kernel, dim3(std::min(nt, FR_GRID_MAX)), dim3(FR_THREADS), 0, stream, (const u8 *)d_stream, (u64)size, nt, tiles);
  hipLaunchKernelGGL(zh_frames_sums_kernel, dim3(1), dim3(FR_THREADS), 0, stream, tiles, nt, ctl);
  return hipGetLastError();
}

hipError_t frames_reach_launch(const void *d_stream, size_t size, size_t max_frames, size_t ncand, u8 *base, hipEvent_t *split,
                               hipStream_t stream) {
  FramesLayout const L = FramesLayout::make(size, max_frames);
  FramesCtl *const ctl = (FramesCtl *)(base + L.ctl);
  u32 const nt = (u32)fr_tiles(size, (uintptr_t)d_stream & 15u), nc = (u32)ncand;
  u64 *const cand = (u64 *)(base + L.cand), *const fsize = (u64 *)(base + L.fsize), *const ffcs = (u64 *)(base + L.ffcs);
  u32 *const info = (u32 *)(base + L.info), *const next = (u32 *)(base + L.next), *const rank = (u32 *)(base + L.rank);
  u32 *ja = (u32 *)(base + L.jump_a), *jb = (u32 *)(base + L.jump_b);
  auto mark = [&](int i) { if (split) (void)hipEventRecord(split[i], stream); };
  mark(0);
  hipLaunchKernelGGL(zh_frames_write_kernel, dim3(std::min(nt, FR_GRID_MAX)), dim3(FR_THREADS), 0, stream, (const u8 *)d_stream, (u64)size, nt,
                     (const u32 *)(base + L.tiles), (u64)ncand, cand);
  mark(1);
  u32 const grid = fr_grid((u64)nc + 2);
  hipLaunchKernelGGL(zh_frames_span_kernel, dim3(grid), dim3(FR_THREADS), 0, stream, (const u8 *)d_stream, (u64)size, nc, cand, fsize, ffcs, info,
                     next, ja, rank);
  mark(2);
  for (u32 k = 0; (1ull << k) < (u64)nc + 2; k++) {  // ceil(log2(nc + 2)) rounds: every distance from candidate 0 is below 2^rounds
    hipLaunchKernelGGL(zh_frames_reach_kernel, dim3(grid), dim3(FR_THREADS), 0, stream, nc, k, ja, jb, rank);
    std::swap(ja, jb);
  }
  mark(3);
  hipLaunchKernelGGL(zh_frames_collect_kernel, dim3(grid), dim3(FR_THREADS), 0, stream, (const u8 *)d_stream, nc, cand, fsize, ffcs, info, next,
                     rank, ctl, frames_out(base, L, max_frames));
  mark(4);
  return hipGetLastError();
}

hipError_t frames_walk_launch(const void *d_stream, size_t size, size_t max_frames, u8 *base, hipStream_t stream) {
  FramesLayout const L = FramesLayout::make(size, max_frames);
  hipLaunchKernelGGL(zh_frames_walk_kernel, dim3(1), dim3(64), 0, stream, (const u8 *)d_stream, (u64)size, (FramesCtl *)(base + L.ctl),
                     frames_out(base, L, max_frames));
  return hipGetLastError();
}

hipError_t frames_sizes_launch(const void *d_stream, size_t size, size_t max_frames, u32 njobs, u8 *base, hipStream_t stream) {
  FramesLayout const L = FramesLayout::make(size, max_frames);
  hipLaunchKernelGGL(zh_frames_sizes_kernel, dim3(fr_grid(njobs)), dim3(FR_THREADS), 0, stream, (const u8 *)d_stream, njobs,
                     (const void *const *)(base + L.in_ptrs), (const size_t *)(base + L.out_sizes), (const int *)(base + L.statuses),
                     (const u32 *)(base + L.job_entry), (u32 *)(base + L.entry_d), (FramesCtl *)(base + L.ctl));
  return hipGetLastError();
}

hipError_t frames_emit_launch(size_t size, size_t max_frames, size_t nframes, void *d_table, u8 *base, hipStream_t stream) {
  FramesLayout const L = FramesLayout::make(size, max_frames);
  hipLaunchKernelGGL(zh_frames_emit_kernel, dim3(fr_grid(nframes)), dim3(FR_THREADS), 0, stream, (u64)nframes, (const u32 *)(base + L.entry_c),
                     (const u32 *)(base + L.entry_d), (u8 *)d_table);
  return hipGetLastError();
}

}  // namespace zh

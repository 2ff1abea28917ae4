// zh_seek.hip — Zstandard seekable streams on the device (format: zh_seek_format.h).
//
// Pack: the N frames a batched compress left in N slots become one contiguous stream followed
// by the seek table.
//   zh_seek_pack_tile_kernel   : validates the items and scans one 1024-item tile of frame sizes
//                                (tile-local exclusive prefix + the tile's sum)
//   zh_seek_pack_sums_kernel   : one workgroup scans the tile sums, decides the call's status,
//                                writes *d_out_size / *d_status and the table's header and footer
//   zh_seek_pack_copy_kernel   : one workgroup per (frame, 16 KiB piece); the tile's base is
//                                added back here, where the offset is used
//   zh_seek_pack_entries*_kernel: the table's entries (with checksums: one wave per frame)
// Read: the table is parsed, validated and scanned on the device, and turned into the job
// arrays of the batched decoder; a last kernel checks the decodes and trims the edge frames.
// Read of many ranges (arithmetic: zh_seek_ranges.h): the same table scan, then
//   zh_seek_ranges_mark_kernel   : one wave per range: verdict, first and last entry, entry bitmap
//   zh_seek_ranges_jobs_kernel   : one decode job into a staging slot per marked entry with content
//   zh_seek_ranges_check_kernel  : one wave per job: the trim kernel's check of the decode
//   zh_seek_ranges_status_kernel : one wave per range: the lowest failing frame's code
//   zh_seek_ranges_scatter_kernel: one workgroup per (range, 16 KiB piece): staging -> destination
#include "zh_common.h"
#include "zh_scan.h"
#include "zh_seek.h"
#include "zh_seek_ranges.h"
#include "zh_xxh64.h"

#include <algorithm>

namespace {

constexpr u32 SK_THREADS = ZH_SCAN_THREADS;
constexpr u32 SK_PER_THREAD = 4;
constexpr u32 SK_TILE = SK_THREADS * SK_PER_THREAD;  // items per scan tile
constexpr u32 SK_PIECE = 16384;                      // bytes per copy workgroup: 256 lanes x 16 B x 4
constexpr u64 SK_NONE = ~0ull;
static_assert(SK_TILE == ZH_SEEK_TILE && SK_PIECE == ZH_SEEK_PIECE, "zh_seek_ranges.h states the tile and the piece");

__host__ __device__ inline size_t sk_align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t sk_tiles(size_t n) { return (n + SK_TILE - 1) / SK_TILE; }

struct PackCtl {
  u64 total;  // bytes of the frames
  u32 ok;
};

struct JobMeta {
  u32 frame;
  u32 flags;  // bit 0: bounced; bit 1: the bounce slot
  u64 dstart;
};

struct RangeJobMeta {  // a batched read's job, in the same array
  u32 frame;
  u32 code;  // the check kernel's verdict
};
static_assert(sizeof(RangeJobMeta) <= sizeof(JobMeta), "the meta array is sized for JobMeta");

__device__ __forceinline__ u64 block_min64(u64 v, u64 *lds) {
  u32 const tid = threadIdx.x;
#pragma unroll
  for (u32 o = 32; o; o >>= 1) {
    u64 const t = __shfl_down((unsigned long long)v, o, 64);
    v = t < v ? t : v;
  }
  __syncthreads();
  if ((tid & 63u) == 0) lds[tid >> 6] = v;
  __syncthreads();
  u64 m = lds[0];
#pragma unroll
  for (u32 k = 1; k < SK_THREADS / 64; k++) m = lds[k] < m ? lds[k] : m;
  return m;
}

// Copy n bytes to an arbitrary destination offset with NT threads: bytes up to the first
// 16-byte boundary of the destination, then 16 bytes per lane at aligned addresses, then the
// tail bytes.  The source is read as aligned dwords realigned with alignbyte; every dword loaded
// holds at least one byte of [src, src + n), every byte stored lies in [dst, dst + n).
template <u32 NT>
__device__ __forceinline__ void copy_bytes(u8 *dst, const u8 *src, u32 n, u32 tid) {
  u32 const h = min((u32)((16u - ((uintptr_t)dst & 15u)) & 15u), n);
  u32 const nv = (n - h) >> 4;
  const u8 *const s0 = src + h;
  u32 const sa = (u32)((uintptr_t)s0 & 3u);
  const u32 *const s32 = (const u32 *)(s0 - sa);
  uint4 *const d16 = (uint4 *)(dst + h);
#pragma unroll 2
  for (u32 k = tid; k < nv; k += NT) {
    const u32 *const q = s32 + 4 * (size_t)k;
    u32 const a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3];
    u32 const a4 = sa ? q[4] : 0u;  // word 4 holds a source byte only when sa != 0
    uint4 v;
    v.x = __builtin_amdgcn_alignbyte(a1, a0, sa);
    v.y = __builtin_amdgcn_alignbyte(a2, a1, sa);
    v.z = __builtin_amdgcn_alignbyte(a3, a2, sa);
    v.w = __builtin_amdgcn_alignbyte(a4, a3, sa);
    d16[k] = v;
  }
  if (tid < h) dst[tid] = src[tid];
  u32 const t0 = h + 16u * nv;  // tail: fewer than 16 bytes
  if (tid < n - t0) dst[t0 + tid] = src[t0 + tid];
}

// A decoded job against the table, by one wave: the decoder's status, the produced size and,
// when asked and the table has them, the checksum over the whole frame at `got`.  e: the
// frame's table entry.  Returns the job's code (0: good), the same in every lane.
__device__ __forceinline__ u32 check_job(const u8 *e, u32 entry, const u8 *got, int status, u64 produced, int verify, u64 *xb) {
  u64 const d = zh_seek_ld32(e + 4);
  u32 code = (u32)status;
  if (code == 0 && produced != d) code = ZH_SEEK_CORRUPT;
  if (code == 0 && verify && entry == 12) {
    u64 const h = zh_xxh64_wave(got, d, xb);
    if ((u32)h != zh_seek_ld32(e + 8)) code = ZH_SEEK_CHECKSUM;
  }
  return code;
}

__device__ __forceinline__ u64 wave_min64(u64 v) {
#pragma unroll
  for (u32 o = 32; o; o >>= 1) {
    u64 const t = __shfl_xor((unsigned long long)v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// Pack
// ---------------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(256) void zh_seek_pack_tile_kernel(const size_t *__restrict__ sizes, const int *__restrict__ statuses,
                                                                           const size_t *__restrict__ usizes, u32 n, u64 max_chunk,
                                                                           u64 *__restrict__ loc, u64 *__restrict__ tsum,
                                                                           u64 *__restrict__ terr) {
  __shared__ u64 lds[4];
  u32 const tid = threadIdx.x;
  u64 const i0 = (u64)blockIdx.x * SK_TILE + (u64)tid * SK_PER_THREAD;
  u64 v[SK_PER_THREAD];
  u64 err = SK_NONE, sum = 0;
#pragma unroll
  for (u32 j = 0; j < SK_PER_THREAD; j++) {
    u64 const i = i0 + j;
    v[j] = 0;
    if (i < n) {
      u64 const s = sizes[i], us = usizes[i];
      u32 code = statuses ? (u32)statuses[i] : 0u;
      if (code) code = (code & 0xFFu) ? (code & 0xFFu) : 1u;
      else if (s == 0 || s > max_chunk || !zh_seek_field_ok(s) || !zh_seek_field_ok(us)) code = ZH_SEEK_INVALID;
      if (code) err = min(err, i << 8 | code);
      else v[j] = s;
    }
    sum += v[j];
  }
  u64 total;
  u64 ex = block_scan_excl64(sum, lds, total);
#pragma unroll
  for (u32 j = 0; j < SK_PER_THREAD; j++) {
    if (i0 + j < n) loc[i0 + j] = ex;
    ex += v[j];
  }
  u64 const e = block_min64(err, lds);
  if (tid == 0) {
    tsum[blockIdx.x] = total;
    terr[blockIdx.x] = e;
  }
}

extern "C" __global__ __launch_bounds__(256) void zh_seek_pack_sums_kernel(const u64 *__restrict__ tsum, const u64 *__restrict__ terr,
                                                                           u64 *__restrict__ tbase, u32 ntiles, u64 n, int with_checksums,
                                                                           u8 *d_out, u64 out_capacity, size_t *d_out_size, int *d_status,
                                                                           PackCtl *ctl) {
  __shared__ u64 lds[4];
  u32 const tid = threadIdx.x;
  u64 carry = 0, err = SK_NONE;
  for (u32 c0 = 0; c0 < ntiles; c0 += SK_THREADS) {
    u32 const t = c0 + tid;
    u64 const v = t < ntiles ? tsum[t] : 0ull;
    if (t < ntiles) err = min(err, terr[t]);
    u64 total;
    u64 const ex = block_scan_excl64(v, lds, total);
    if (t < ntiles) tbase[t] = carry + ex;
    carry += total;
  }
  err = block_min64(err, lds);
  if (tid == 0) {
    u64 const table = zh_seek_table_bytes(n, with_checksums);
    u32 code = ZH_SEEK_OK;
    if (err != SK_NONE) code = (u32)(err & 0xFFu);  // the first failing item's code
    else if (carry + table > out_capacity) code = ZH_SEEK_TOO_SMALL;
    ctl->total = carry;
    ctl->ok = code == ZH_SEEK_OK;
    *d_out_size = code == ZH_SEEK_OK ? (size_t)(carry + table) : 0;
    *d_status = (int)code;
    if (code == ZH_SEEK_OK) {
      zh_seek_write_header(d_out + carry, n, with_checksums);
      zh_seek_write_footer(d_out + carry + 8 + n * zh_seek_entry_bytes(with_checksums), n, with_checksums);
    }
  }
}

extern "C" __global__ __launch_bounds__(256) void zh_seek_pack_copy_kernel(const void *const *__restrict__ ptrs, const size_t *__restrict__ sizes,
                                                                           const u64 *__restrict__ loc, const u64 *__restrict__ tbase,
                                                                           const PackCtl *__restrict__ ctl, u32 n, u32 ppf, u8 *d_out) {
  if (!ctl->ok) return;
  u64 const nwork = (u64)n * ppf;
  for (u64 w = blockIdx.x; w < nwork; w += gridDim.x) {
    u32 const f = (u32)(w / ppf), p = (u32)(w % ppf);
    u64 const sz = sizes[f], po = (u64)p * SK_PIECE;
    if (po >= sz) continue;
    u32 const cnt = (u32)min((u64)SK_PIECE, sz - po);
    copy_bytes<SK_THREADS>(d_out + tbase[f / SK_TILE] + loc[f] + po, (const u8 *)ptrs[f] + po, cnt, threadIdx.x);
  }
}

extern "C" __global__ __launch_bounds__(256) void zh_seek_pack_entries_kernel(const size_t *__restrict__ sizes, const size_t *__restrict__ usizes,
                                                                              u32 n, const PackCtl *__restrict__ ctl, u8 *d_out) {
  if (!ctl->ok) return;
  u64 const i = (u64)blockIdx.x * SK_THREADS + threadIdx.x;
  if (i >= n) return;
  zh_seek_write_entry(d_out + ctl->total + 8 + i * 8, (u32)sizes[i], (u32)usizes[i], 0, 0);
}

// With checksums: one wave per frame hashes the uncompressed chunk.
extern "C" __global__ __launch_bounds__(256) void zh_seek_pack_entries_ck_kernel(const size_t *__restrict__ sizes,
                                                                                 const void *const *__restrict__ uptrs,
                                                                                 const size_t *__restrict__ usizes, u32 n,
                                                                                 const PackCtl *__restrict__ ctl, u8 *d_out) {
  __shared__ u64 xb[SK_THREADS / 64][512];
  if (!ctl->ok) return;
  u32 const wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  u64 const i = (u64)blockIdx.x * (SK_THREADS / 64) + wave;
  if (i >= n) return;
  u64 const us = usizes[i];
  u64 const h = zh_xxh64_wave((const u8 *)uptrs[i], us, xb[wave]);
  if (lane == 0) zh_seek_write_entry(d_out + ctl->total + 8 + i * 12, (u32)sizes[i], (u32)us, 1, (u32)h);
}

// ---------------------------------------------------------------------------------------------
// Read
// ---------------------------------------------------------------------------------------------
// One tile of the table: field limits, tile-local exclusive scans of both columns, tile sums.
extern "C" __global__ __launch_bounds__(256) void zh_seek_index_tile_kernel(const u8 *__restrict__ stream, u64 size, u32 n,
                                                                            u64 *__restrict__ lc, u64 *__restrict__ ld, u64 *__restrict__ tcs,
                                                                            u64 *__restrict__ tds, zh::SeekReadCtl *ctl) {
  __shared__ u64 lds[4];
  u32 const tid = threadIdx.x;
  ZhSeekFooter f;
  u32 code = zh_seek_parse_footer(stream + size - ZH_SEEK_FOOTER, size, &f);  // the host checked size >= 17
  if (code == ZH_SEEK_OK && f.n != n) code = ZH_SEEK_CORRUPT;
  if (code != ZH_SEEK_OK) {  // uniform over the grid: no table to trust, no entry is read
    if (blockIdx.x == 0 && tid == 0) ctl->status = code;
    return;
  }
  const u8 *const table = stream + (size - f.table);
  if (blockIdx.x == 0 && tid == 0 && zh_seek_check_header(table, &f) != ZH_SEEK_OK) atomicOr(&ctl->bad, 1u);
  u64 const i0 = (u64)blockIdx.x * SK_TILE + (u64)tid * SK_PER_THREAD;
  u64 c[SK_PER_THREAD], d[SK_PER_THREAD];
  u64 sc = 0, sd = 0;
  u32 mx = 0, bad = 0;
#pragma unroll
  for (u32 j = 0; j < SK_PER_THREAD; j++) {
    c[j] = d[j] = 0;
    if (i0 + j < n) {
      const u8 *const e = table + 8 + (i0 + j) * f.entry;
      c[j] = zh_seek_ld32(e);
      d[j] = zh_seek_ld32(e + 4);
      if (!zh_seek_field_ok(c[j]) || !zh_seek_field_ok(d[j])) { bad = 1; c[j] = d[j] = 0; }
      mx = max(mx, (u32)d[j]);
    }
    sc += c[j];
    sd += d[j];
  }
  u64 tc, td;
  u64 ec = block_scan_excl64(sc, lds, tc);
  u64 ed = block_scan_excl64(sd, lds, td);
#pragma unroll
  for (u32 j = 0; j < SK_PER_THREAD; j++) {
    if (i0 + j < n) { lc[i0 + j] = ec; ld[i0 + j] = ed; }
    ec += c[j];
    ed += d[j];
  }
  if (tid == 0 && n) { tcs[blockIdx.x] = tc; tds[blockIdx.x] = td; }  // (n == 0: one workgroup, no tile)
  if (mx) atomicMax(&ctl->max_d, mx);
  if (bad) atomicOr(&ctl->bad, 1u);
}

// Scan of the tile sums; the call's verdict on the table and on the range.
extern "C" __global__ __launch_bounds__(256) void zh_seek_index_sums_kernel(u64 *__restrict__ tcs, u64 *__restrict__ tds, u32 ntiles, u64 size,
                                                                            u64 table_bytes, u64 offset, u64 length, zh::SeekReadCtl *ctl) {
  __shared__ u64 lds[4];
  u32 const tid = threadIdx.x;
  u64 cc = 0, cd = 0;
  for (u32 c0 = 0; c0 < ntiles; c0 += SK_THREADS) {  // in place: sums become exclusive bases
    u32 const t = c0 + tid;
    u64 const vc = t < ntiles ? tcs[t] : 0ull, vd = t < ntiles ? tds[t] : 0ull;
    u64 tc, td;
    u64 const ec = block_scan_excl64(vc, lds, tc);
    u64 const ed = block_scan_excl64(vd, lds, td);
    if (t < ntiles) { tcs[t] = cc + ec; tds[t] = cd + ed; }
    cc += tc;
    cd += td;
  }
  if (tid == 0) {
    u32 code = ctl->status;
    if (code == ZH_SEEK_OK) {
      if (ctl->bad || cc + table_bytes != size) code = ZH_SEEK_CORRUPT;
      else if (offset > cd || length > cd - offset) code = ZH_SEEK_INVALID;
    }
    ctl->status = code;
    ctl->total_c = cc;
    ctl->total_u = cd;
    ctl->errkey = SK_NONE;
  }
}

// One thread per entry: a frame with content inside [offset, offset + length) becomes one job.
// With the table validated (status 0), cstart + csize <= size - table_bytes and, for a frame
// wholly inside the range, dstart - offset + dsize <= length: every pointer stays in its buffer.
extern "C" __global__ __launch_bounds__(256) void zh_seek_index_jobs_kernel(const u8 *__restrict__ stream, u64 size, u32 n, u32 entry,
                                                                            u64 table_bytes, const u64 *__restrict__ lc,
                                                                            const u64 *__restrict__ ld, const u64 *__restrict__ tbc,
                                                                            const u64 *__restrict__ tbd, u64 offset, u64 length, u8 *d_out,
                                                                            u8 *bounce, zh::SeekReadCtl *ctl, zh::SeekJobs jobs) {
  if (ctl->status != ZH_SEEK_OK || length == 0) return;
  u64 const i = (u64)blockIdx.x * SK_THREADS + threadIdx.x;
  if (i >= n) return;
  const u8 *const e = stream + (size - table_bytes) + 8 + i * entry;
  u64 const c = zh_seek_ld32(e), d = zh_seek_ld32(e + 4);
  if (d == 0) return;  // an empty frame, or a skippable frame listed as an entry
  u64 const t = i / SK_TILE;
  u64 const dstart = tbd[t] + ld[i], cstart = tbc[t] + lc[i];
  u64 const end = offset + length;
  if (dstart >= end || dstart + d <= offset) return;
  u32 const j = atomicAdd(&ctl->njobs, 1u);
  bool const partial = dstart < offset || dstart + d > end;
  u32 const slot = dstart < offset ? 0u : 1u;  // at most one frame starts before the range, one ends after it
  jobs.in_ptrs[j] = stream + cstart;
  jobs.in_sizes[j] = (size_t)c;
  jobs.out_ptrs[j] = partial ? bounce + (size_t)slot * sk_align256(ctl->max_d) : d_out + (dstart - offset);
  jobs.out_caps[j] = (size_t)d;
  JobMeta m;
  m.frame = (u32)i;
  m.flags = partial ? 1u | slot << 1 : 0u;
  m.dstart = dstart;
  ((JobMeta *)jobs.meta)[j] = m;
}

// One wave per job: the decoder's status and size against the table, the checksum when asked,
// and the overlap of a bounced edge frame into d_out.
extern "C" __global__ __launch_bounds__(64) void zh_seek_trim_kernel(const u8 *__restrict__ stream, u64 size, u32 entry, u64 table_bytes,
                                                                     u64 offset, u64 length, u8 *d_out, int verify, zh::SeekReadCtl *ctl,
                                                                     zh::SeekJobs jobs) {
  __shared__ u64 xb[512];
  u32 const j = blockIdx.x, lane = threadIdx.x;
  JobMeta const m = ((const JobMeta *)jobs.meta)[j];
  const u8 *const e = stream + (size - table_bytes) + 8 + (u64)m.frame * entry;
  u64 const d = zh_seek_ld32(e + 4);
  const u8 *const got = (const u8 *)jobs.out_ptrs[j];
  u32 const code = check_job(e, entry, got, jobs.statuses[j], jobs.out_sizes[j], verify, xb);  // an edge frame: over the bounce slot's full frame
  if (code) {
    if (lane == 0) atomicMin((unsigned long long *)&ctl->errkey, (unsigned long long)((u64)m.frame << 8 | (code & 0xFFu)));
    return;
  }
  if (m.flags & 1u) {
    u64 const lo = max(m.dstart, offset), hi = min(m.dstart + d, offset + length);
    copy_bytes<64>(d_out + (lo - offset), got + (lo - m.dstart), (u32)(hi - lo), lane);
  }
}

// ---------------------------------------------------------------------------------------------
// Read of many ranges: the table is scanned once (the two index kernels above), every frame a
// range touches is decoded once into a staging slot, and each range's bytes are copied from the
// slots to its destination.
// ---------------------------------------------------------------------------------------------
// One wave per range: its verdict (kept in first[]), its first and last entry, and the bits of
// the entries between them.
extern "C" __global__ __launch_bounds__(256) void zh_seek_ranges_mark_kernel(const u64 *__restrict__ offsets, const size_t *__restrict__ lengths,
                                                                             u64 nranges, u64 max_length, u32 n, const u64 *__restrict__ ld,
                                                                             const u64 *__restrict__ tbd, const zh::SeekReadCtl *__restrict__ ctl,
                                                                             u32 *__restrict__ first, u32 *__restrict__ last, u32 *bitmap) {
  if (ctl->status != ZH_SEEK_OK) return;  // no table to trust
  u32 const wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  ZhSeekIndex const x{ld, tbd, n, ctl->total_u};
  u64 const nwaves = (u64)gridDim.x * (SK_THREADS / 64);
  for (u64 r = (u64)blockIdx.x * (SK_THREADS / 64) + wave; r < nranges; r += nwaves) {
    u64 const off = offsets[r], len = lengths[r];
    if (!zh_seek_range_ok(off, len, x.total, max_length) || len == 0) {
      if (lane == 0) first[r] = len == 0 && off <= x.total ? ZH_SEEK_RANGE_EMPTY : ZH_SEEK_RANGE_INVALID;
      continue;
    }
    u32 const a = (u32)zh_seek_cover(x, off), b = (u32)zh_seek_cover(x, off + len - 1);
    if (lane == 0) {
      first[r] = a;
      last[r] = b;
    }
    for (u32 w = (a >> 5) + lane; w <= (b >> 5); w += 64) {
      u32 m = ~0u;
      if (w == (a >> 5)) m &= ~0u << (a & 31u);
      if (w == (b >> 5)) m &= ~0u >> (31u - (b & 31u));
      atomicOr(&bitmap[w], m);
    }
  }
}

// One lane per entry: a marked entry with content becomes one decode job into its staging slot.
// The job arrays hold n items and at most n jobs exist; the slot's address is only computed
// here: the host launches the decoder after it has seen that the temp buffer holds njobs slots.
extern "C" __global__ __launch_bounds__(256) void zh_seek_ranges_jobs_kernel(const u8 *__restrict__ stream, u64 size, u32 n, u32 entry,
                                                                             u64 table_bytes, const u64 *__restrict__ lc,
                                                                             const u64 *__restrict__ tbc, const u32 *__restrict__ bitmap,
                                                                             u8 *staging, zh::SeekReadCtl *ctl, zh::SeekJobs jobs,
                                                                             u32 *__restrict__ job_of_frame) {
  if (ctl->status != ZH_SEEK_OK) return;
  u64 const i = (u64)blockIdx.x * SK_THREADS + threadIdx.x;
  if (i >= n || !(bitmap[i >> 5] >> (i & 31u) & 1u)) return;
  const u8 *const e = stream + (size - table_bytes) + 8 + i * entry;
  u64 const c = zh_seek_ld32(e), d = zh_seek_ld32(e + 4);
  if (d == 0) return;  // an empty frame, or a skippable frame listed as an entry
  u32 const j = atomicAdd(&ctl->njobs, 1u);
  jobs.in_ptrs[j] = stream + tbc[i / SK_TILE] + lc[i];
  jobs.in_sizes[j] = (size_t)c;
  jobs.out_ptrs[j] = staging + (size_t)j * sk_align256(ctl->max_d);
  jobs.out_caps[j] = (size_t)d;
  RangeJobMeta m;
  m.frame = (u32)i;
  m.code = 0;
  ((RangeJobMeta *)jobs.meta)[j] = m;
  job_of_frame[i] = j;
}

// One wave per job: the decode against the table (the trim kernel's check).
extern "C" __global__ __launch_bounds__(64) void zh_seek_ranges_check_kernel(const u8 *__restrict__ stream, u64 size, u32 entry, u64 table_bytes,
                                                                             int verify, zh::SeekJobs jobs) {
  __shared__ u64 xb[512];
  u32 const j = blockIdx.x;
  RangeJobMeta *const m = (RangeJobMeta *)jobs.meta + j;
  const u8 *const e = stream + (size - table_bytes) + 8 + (u64)m->frame * entry;
  u32 const code = check_job(e, entry, (const u8 *)jobs.out_ptrs[j], jobs.statuses[j], jobs.out_sizes[j], verify, xb);
  if (threadIdx.x == 0 && code) m->code = (code & 0xFFu) ? (code & 0xFFu) : 1u;
}

// One wave per range: the code of the lowest failing frame it touches, or its own verdict.
extern "C" __global__ __launch_bounds__(256) void zh_seek_ranges_status_kernel(u64 nranges, const u32 *__restrict__ first,
                                                                               const u32 *__restrict__ last, const u32 *__restrict__ job_of_frame,
                                                                               zh::SeekJobs jobs, int *__restrict__ statuses) {
  u32 const wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const RangeJobMeta *const meta = (const RangeJobMeta *)jobs.meta;
  u64 const nwaves = (u64)gridDim.x * (SK_THREADS / 64);
  for (u64 r = (u64)blockIdx.x * (SK_THREADS / 64) + wave; r < nranges; r += nwaves) {
    u32 const a = first[r];
    u32 code = a == ZH_SEEK_RANGE_INVALID ? (u32)ZH_SEEK_INVALID : (u32)ZH_SEEK_OK;
    if (a < ZH_SEEK_RANGE_EMPTY) {
      u64 key = SK_NONE;
      u64 const b = last[r];
      for (u64 i = (u64)a + lane; i <= b; i += 64) {
        u32 const j = job_of_frame[i];
        if (j == ZH_SEEK_NO_JOB) continue;  // an entry of size 0
        u32 const c = meta[j].code;
        if (c) key = min(key, i << 8 | c);
      }
      key = wave_min64(key);
      if (key != SK_NONE) code = (u32)(key & 0xFFu);
    }
    if (lane == 0) statuses[r] = (int)code;
  }
}

// One workgroup per (range, 16 KiB piece of its content): the piece's segments, one per frame
// with content, from the frames' staging slots to the range's destination.
extern "C" __global__ __launch_bounds__(256) void zh_seek_ranges_scatter_kernel(const u64 *__restrict__ offsets, const size_t *__restrict__ lengths,
                                                                                void *const *__restrict__ out_ptrs, const int *__restrict__ statuses,
                                                                                u64 nranges, u32 ppr, u32 n, const u64 *__restrict__ ld,
                                                                                const u64 *__restrict__ tbd, const zh::SeekReadCtl *__restrict__ ctl,
                                                                                const u32 *__restrict__ job_of_frame, const u8 *__restrict__ staging) {
  ZhSeekIndex const x{ld, tbd, n, ctl->total_u};
  size_t const slot = sk_align256(ctl->max_d);
  u64 const nwork = nranges * ppr;
  for (u64 w = blockIdx.x; w < nwork; w += gridDim.x) {
    u64 const r = w / ppr, po = (w % ppr) * SK_PIECE;
    if (statuses[r] != 0) continue;  // a failed range: nothing of its destination is written
    u64 const len = lengths[r];
    if (po >= len) continue;
    u64 const p0 = offsets[r] + po, end = p0 + min((u64)SK_PIECE, len - po);
    u8 *const dst = (u8 *)out_ptrs[r] + po;
    u64 i = zh_seek_cover(x, p0), pos = p0;
    ZhSeekSeg s;
    while (zh_seek_next_seg(x, &i, &pos, end, &s))
      copy_bytes<SK_THREADS>(dst + (s.pos - p0), staging + (size_t)job_of_frame[s.frame] * slot + s.in_frame, (u32)s.len, threadIdx.x);
  }
}

// Totals of a table (the info call): per-workgroup reductions, then one atomic each.
extern "C" __global__ __launch_bounds__(256) void zh_seek_info_kernel(const u8 *__restrict__ stream, u64 size, u32 n, zh::SeekInfoRes *res) {
  __shared__ u64 lds[4];
  u32 const tid = threadIdx.x;
  ZhSeekFooter f;
  if (zh_seek_parse_footer(stream + size - ZH_SEEK_FOOTER, size, &f) != ZH_SEEK_OK || f.n != n) {
    if (blockIdx.x == 0 && tid == 0) atomicOr(&res->bad, 1u);
    return;
  }
  const u8 *const table = stream + (size - f.table);
  if (blockIdx.x == 0 && tid == 0 && zh_seek_check_header(table, &f) != ZH_SEEK_OK) atomicOr(&res->bad, 1u);
  u64 sc = 0, sd = 0;
  u32 mx = 0, bad = 0;
  for (u64 i = (u64)blockIdx.x * SK_THREADS + tid; i < n; i += (u64)gridDim.x * SK_THREADS) {
    const u8 *const e = table + 8 + i * f.entry;
    u64 const c = zh_seek_ld32(e), d = zh_seek_ld32(e + 4);
    if (!zh_seek_field_ok(c) || !zh_seek_field_ok(d)) { bad = 1; continue; }
    sc += c;
    sd += d;
    mx = max(mx, (u32)d);
  }
  u64 tc, td;
  (void)block_scan_excl64(sc, lds, tc);
  (void)block_scan_excl64(sd, lds, td);
  if (tid == 0) {
    atomicAdd((unsigned long long *)&res->total_c, (unsigned long long)tc);
    atomicAdd((unsigned long long *)&res->total_u, (unsigned long long)td);
  }
  if (mx) atomicMax(&res->max_d, mx);
  if (bad) atomicOr(&res->bad, 1u);
}

// ---------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------
namespace zh {

namespace {
struct PackLayout {
  size_t ctl, loc, tsum, terr, tbase, total;
  static PackLayout make(size_t n) {
    PackLayout L{};
    size_t const t = sk_tiles(n);
    size_t o = 0;
    L.ctl = o; o = sk_align256(o + sizeof(PackCtl));
    L.loc = o; o = sk_align256(o + n * 8);
    L.tsum = o; o = sk_align256(o + t * 8);
    L.terr = o; o = sk_align256(o + t * 8);
    L.tbase = o; o = sk_align256(o + t * 8);
    L.total = o + 256;  // slack for base alignment
    return L;
  }
};

struct ReadLayout {
  size_t ctl, lc, ld, tbc, tbd, in_ptrs, in_sizes, out_ptrs, out_caps, out_sizes, statuses, meta, total;
  static ReadLayout make(size_t n) {
    ReadLayout L{};
    size_t const t = sk_tiles(n);
    size_t o = 0;
    L.ctl = o; o = sk_align256(o + sizeof(SeekReadCtl));
    L.lc = o; o = sk_align256(o + n * 8);
    L.ld = o; o = sk_align256(o + n * 8);
    L.tbc = o; o = sk_align256(o + t * 8);
    L.tbd = o; o = sk_align256(o + t * 8);
    L.in_ptrs = o; o = sk_align256(o + n * 8);
    L.in_sizes = o; o = sk_align256(o + n * 8);
    L.out_ptrs = o; o = sk_align256(o + n * 8);
    L.out_caps = o; o = sk_align256(o + n * 8);
    L.out_sizes = o; o = sk_align256(o + n * 8);
    L.statuses = o; o = sk_align256(o + n * 4);
    L.meta = o; o = sk_align256(o + n * sizeof(JobMeta));
    L.total = o;
    return L;
  }
};
}  // namespace

size_t seek_pack_temp_bytes(size_t n) { return PackLayout::make(n).total; }

hipError_t seek_pack_launch(const void *const *d_frame_ptrs, const size_t *d_frame_sizes, const int *d_frame_statuses,
                            const void *const *d_uncompressed_ptrs, const size_t *d_uncompressed_sizes, size_t n,
                            size_t max_compressed_chunk_bytes, int with_checksums, void *d_out, size_t out_capacity, size_t *d_out_size,
                            int *d_status, void *d_temp, hipStream_t stream) {
  PackLayout const L = PackLayout::make(n);
  u8 *const base = (u8 *)(((uintptr_t)d_temp + 255) & ~(uintptr_t)255);
  PackCtl *const ctl = (PackCtl *)(base + L.ctl);
  u64 *const loc = (u64 *)(base + L.loc), *const tsum = (u64 *)(base + L.tsum), *const terr = (u64 *)(base + L.terr),
             *const tbase = (u64 *)(base + L.tbase);
  u32 const nt = (u32)sk_tiles(n);
  if (nt)
    hipLaunchKernelGGL(zh_seek_pack_tile_kernel, dim3(nt), dim3(SK_THREADS), 0, stream, d_frame_sizes, d_frame_statuses, d_uncompressed_sizes,
                       (u32)n, (u64)max_compressed_chunk_bytes, loc, tsum, terr);
  hipLaunchKernelGGL(zh_seek_pack_sums_kernel, dim3(1), dim3(SK_THREADS), 0, stream, tsum, terr, tbase, nt, (u64)n, with_checksums, (u8 *)d_out,
                     (u64)out_capacity, d_out_size, d_status, ctl);
  if (n) {
    u64 const ppf = std::max<u64>(1, ((u64)max_compressed_chunk_bytes + SK_PIECE - 1) / SK_PIECE);
    u32 const grid = (u32)std::min<u64>((u64)n * ppf, 1u << 22);  // larger batches stride the grid
    hipLaunchKernelGGL(zh_seek_pack_copy_kernel, dim3(grid), dim3(SK_THREADS), 0, stream, d_frame_ptrs, d_frame_sizes, loc, tbase, ctl, (u32)n,
                       (u32)std::min<u64>(ppf, 0xFFFFFFFFull), (u8 *)d_out);
    if (with_checksums)
      hipLaunchKernelGGL(zh_seek_pack_entries_ck_kernel, dim3((u32)((n + 3) / 4)), dim3(SK_THREADS), 0, stream, d_frame_sizes,
                         d_uncompressed_ptrs, d_uncompressed_sizes, (u32)n, ctl, (u8 *)d_out);
    else
      hipLaunchKernelGGL(zh_seek_pack_entries_kernel, dim3((u32)((n + SK_THREADS - 1) / SK_THREADS)), dim3(SK_THREADS), 0, stream, d_frame_sizes,
                         d_uncompressed_sizes, (u32)n, ctl, (u8 *)d_out);
  }
  return hipGetLastError();
}

size_t seek_read_fixed_bytes(size_t n) { return ReadLayout::make(n).total; }
size_t seek_read_bounce_bytes(size_t max_d) { return 2 * sk_align256(std::max<size_t>(max_d, 1)); }

SeekJobs seek_read_jobs(u8 *base, size_t n) {
  ReadLayout const L = ReadLayout::make(n);
  SeekJobs j;
  j.in_ptrs = (const void **)(base + L.in_ptrs);
  j.in_sizes = (size_t *)(base + L.in_sizes);
  j.out_ptrs = (void **)(base + L.out_ptrs);
  j.out_caps = (size_t *)(base + L.out_caps);
  j.out_sizes = (size_t *)(base + L.out_sizes);
  j.statuses = (int *)(base + L.statuses);
  j.meta = base + L.meta;
  return j;
}

// The control block zeroed, then the two scan kernels: the table's verdict, and the range's when
// one is given (a batched read gives offset 0, length 0 and judges its ranges itself).
static hipError_t seek_scan_launch(const void *d_stream, size_t size, size_t n, u32 entry, u64 offset, u64 length, u8 *base, hipStream_t stream) {
  ReadLayout const L = ReadLayout::make(n);
  SeekReadCtl *const ctl = (SeekReadCtl *)(base + L.ctl);
  u64 *const tbc = (u64 *)(base + L.tbc), *const tbd = (u64 *)(base + L.tbd);
  hipError_t e = hipMemsetAsync(ctl, 0, sizeof(SeekReadCtl), stream);
  if (e != hipSuccess) return e;
  u32 const nt = (u32)sk_tiles(n);
  // (n == 0: the footer is still parsed on the device, by one workgroup that finds no entry)
  hipLaunchKernelGGL(zh_seek_index_tile_kernel, dim3(std::max(nt, 1u)), dim3(SK_THREADS), 0, stream, (const u8 *)d_stream, (u64)size, (u32)n,
                     (u64 *)(base + L.lc), (u64 *)(base + L.ld), tbc, tbd, ctl);
  hipLaunchKernelGGL(zh_seek_index_sums_kernel, dim3(1), dim3(SK_THREADS), 0, stream, tbc, tbd, n ? nt : 0u, (u64)size,
                     (u64)n * entry + ZH_SEEK_OVERHEAD, offset, length, ctl);
  return hipSuccess;
}

hipError_t seek_index_launch(const void *d_stream, size_t size, size_t n, u32 entry, u64 offset, u64 length, void *d_out, u8 *base,
                             hipStream_t stream) {
  ReadLayout const L = ReadLayout::make(n);
  SeekReadCtl *const ctl = (SeekReadCtl *)(base + L.ctl);
  u64 *const lc = (u64 *)(base + L.lc), *const ld = (u64 *)(base + L.ld), *const tbc = (u64 *)(base + L.tbc), *const tbd = (u64 *)(base + L.tbd);
  hipError_t const e = seek_scan_launch(d_stream, size, n, entry, offset, length, base, stream);
  if (e != hipSuccess) return e;
  u64 const table_bytes = (u64)n * entry + ZH_SEEK_OVERHEAD;
  if (n)
    hipLaunchKernelGGL(zh_seek_index_jobs_kernel, dim3((u32)((n + SK_THREADS - 1) / SK_THREADS)), dim3(SK_THREADS), 0, stream,
                       (const u8 *)d_stream, (u64)size, (u32)n, entry, table_bytes, lc, ld, tbc, tbd, offset, length, (u8 *)d_out, base + L.total,
                       ctl, seek_read_jobs(base, n));
  return hipGetLastError();
}

hipError_t seek_trim_launch(const void *d_stream, size_t size, size_t n, u32 entry, u32 njobs, u64 offset, u64 length, void *d_out, int verify,
                            u8 *base, hipStream_t stream) {
  if (!njobs) return hipSuccess;
  ReadLayout const L = ReadLayout::make(n);
  hipLaunchKernelGGL(zh_seek_trim_kernel, dim3(njobs), dim3(64), 0, stream, (const u8 *)d_stream, (u64)size, entry,
                     (u64)n * entry + ZH_SEEK_OVERHEAD, offset, length, (u8 *)d_out, verify, (SeekReadCtl *)(base + L.ctl), seek_read_jobs(base, n));
  return hipGetLastError();
}

ZhSeekRangesLayout seek_ranges_layout(size_t n, size_t num_ranges, size_t jobs, size_t max_d, size_t dec_bytes) {
  return zh_seek_ranges_layout(ReadLayout::make(n).total, n, num_ranges, jobs, max_d, dec_bytes);
}

hipError_t seek_ranges_index_launch(const void *d_stream, size_t size, size_t n, u32 entry, const unsigned long long *d_offsets,
                                    const size_t *d_lengths, size_t num_ranges, size_t max_length, u8 *base, hipStream_t stream) {
  ReadLayout const L = ReadLayout::make(n);
  ZhSeekRangesLayout const R = seek_ranges_layout(n, num_ranges, 0, 0, 0);
  SeekReadCtl *const ctl = (SeekReadCtl *)(base + L.ctl);
  const u64 *const lc = (const u64 *)(base + L.lc), *const ld = (const u64 *)(base + L.ld), *const tbc = (const u64 *)(base + L.tbc),
                   *const tbd = (const u64 *)(base + L.tbd);
  u32 *const bitmap = (u32 *)(base + R.bitmap), *const jof = (u32 *)(base + R.job_of_frame);
  // (offset 0, length 0: the table's verdict alone; the ranges get theirs from the mark kernel)
  hipError_t e = seek_scan_launch(d_stream, size, n, entry, 0, 0, base, stream);
  if (e != hipSuccess) return e;
  u64 const table_bytes = (u64)n * entry + ZH_SEEK_OVERHEAD;
  if (n) {
    if ((e = hipMemsetAsync(bitmap, 0, R.bitmap_bytes, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(jof, 0xFF, n * 4, stream)) != hipSuccess) return e;
  }
  u32 const rgrid = (u32)std::min<u64>(((u64)num_ranges + 3) / 4, 1u << 20);  // more ranges stride the grid
  hipLaunchKernelGGL(zh_seek_ranges_mark_kernel, dim3(rgrid), dim3(SK_THREADS), 0, stream, (const u64 *)d_offsets, d_lengths, (u64)num_ranges,
                     (u64)max_length, (u32)n, ld, tbd, ctl, (u32 *)(base + R.first), (u32 *)(base + R.last), bitmap);
  if (n)
    hipLaunchKernelGGL(zh_seek_ranges_jobs_kernel, dim3((u32)((n + SK_THREADS - 1) / SK_THREADS)), dim3(SK_THREADS), 0, stream,
                       (const u8 *)d_stream, (u64)size, (u32)n, entry, table_bytes, lc, tbc, bitmap, base + R.staging, ctl, seek_read_jobs(base, n),
                       jof);
  return hipGetLastError();
}

hipError_t seek_ranges_finish_launch(const void *d_stream, size_t size, size_t n, u32 entry, u32 njobs, const unsigned long long *d_offsets,
                                     const size_t *d_lengths, void *const *d_out_ptrs, size_t num_ranges, size_t max_length, int verify,
                                     int *d_range_statuses, u8 *base, hipStream_t stream) {
  ReadLayout const L = ReadLayout::make(n);
  ZhSeekRangesLayout const R = seek_ranges_layout(n, num_ranges, 0, 0, 0);
  SeekJobs const jobs = seek_read_jobs(base, n);
  const u32 *const jof = (const u32 *)(base + R.job_of_frame);
  if (njobs)
    hipLaunchKernelGGL(zh_seek_ranges_check_kernel, dim3(njobs), dim3(64), 0, stream, (const u8 *)d_stream, (u64)size, entry,
                       (u64)n * entry + ZH_SEEK_OVERHEAD, verify, jobs);
  u32 const rgrid = (u32)std::min<u64>(((u64)num_ranges + 3) / 4, 1u << 20);
  hipLaunchKernelGGL(zh_seek_ranges_status_kernel, dim3(rgrid), dim3(SK_THREADS), 0, stream, (u64)num_ranges, (const u32 *)(base + R.first),
                     (const u32 *)(base + R.last), jof, jobs, d_range_statuses);
  if (njobs && max_length) {
    u64 const ppr = std::min<u64>(((u64)max_length + SK_PIECE - 1) / SK_PIECE, 0xFFFFFFFFull);
    u32 const grid = (u32)std::min<u64>((u64)num_ranges * ppr, 1u << 22);  // larger batches stride the grid
    hipLaunchKernelGGL(zh_seek_ranges_scatter_kernel, dim3(grid), dim3(SK_THREADS), 0, stream, (const u64 *)d_offsets, d_lengths, d_out_ptrs,
                       (const int *)d_range_statuses, (u64)num_ranges, (u32)ppr, (u32)n, (const u64 *)(base + L.ld), (const u64 *)(base + L.tbd),
                       (const SeekReadCtl *)(base + L.ctl), jof, (const u8 *)(base + R.staging));
  }
  return hipGetLastError();
}

hipError_t seek_info_launch(const void *d_stream, size_t size, size_t n, SeekInfoRes *d_res, hipStream_t stream) {
  u32 const grid = (u32)std::min<size_t>(std::max<size_t>(sk_tiles(n), 1), 1024);
  hipLaunchKernelGGL(zh_seek_info_kernel, dim3(grid), dim3(SK_THREADS), 0, stream, (const u8 *)d_stream, (u64)size, (u32)n, d_res);
  return hipGetLastError();
}

}  // namespace zh

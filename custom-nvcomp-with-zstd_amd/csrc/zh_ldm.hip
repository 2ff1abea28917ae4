// zh_ldm.hip — long-distance matching for frames of more than one device block (DESIGN.md,
// long-distance matching; the rules are restated in tests/zh_ldm_model.py).
//
// The whole frame is resident, so the index covers all of it at once:
//   zh_ldm_index_kernel : one workgroup per 32 KiB cell hashes every position (zh_ldm.h), keeps
//                         the cell's first ZH_LDM_CELL_SAMPLES samples in position order and
//                         enters them into the table with a 64-bit atomicMin of
//                         position << 32 | tag: the earliest position wins, whatever the order
//                         the workgroups run in.
//   zh_ldm_cell_kernel  : one workgroup per cell looks its samples up, keeps the first
//                         ZH_LDM_CELL_OFFSETS distinct distances beyond K1's reach, finds the
//                         longest run of the cell equal to itself that far back, and writes the
//                         cell's three block descriptors: [gap][one-sequence block][gap].  Gap
//                         blocks go through K1-K4 like any block; the one-sequence block's bytes
//                         and staged size are written here (its slot has n = 0 and ZH_F_LDM).
// Every load is inside [src, src + size); stores are vector stores and global atomics.
#include "zh_common.h"
#include "zh_launch.h"
#include "zh_ldm.h"

#include <mutex>
#include <vector>

#define LDM_THREADS 256u
#define LDM_RUN (ZH_LDM_CELL / LDM_THREADS)  // positions (and run-search bytes) per lane: 128
static_assert(LDM_RUN == 128u, "a lane's sample bits are two u64");
static_assert(ZH_LDM_MIN_SEG >= 2u * LDM_RUN, "the run search is exact only for runs of at least one lane's bytes");
static_assert(ZH_LDM_CELL == ZH_HIST_BLOCK, "cells are the frame's device blocks");
static_assert(ZH_LDM_CELL_SAMPLES == 2u * LDM_THREADS, "two samples per lane in the lookup");

// 16 bytes at p, any alignment (inside the caller's buffer)
__device__ __forceinline__ uint4 ld16(const u8 *p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

// Staged cell: dword w of the cell lives at LDS dword w + (w >> 5).  A lane reads the 48 dwords
// from 32 * lane on: unpadded, every lane of a wave would sit on one bank; with one pad dword per
// 32 the lanes' k-th dwords fall on 32 consecutive banks.
#define LDM_STAGE_WORDS ((ZH_LDM_CELL + 64u) / 4u)
#define LDM_PAD(w) ((w) + ((w) >> 5))
#define LDM_STAGE_LDS (LDM_PAD(LDM_STAGE_WORDS) + 1u)

__device__ __forceinline__ u32 block_scan_excl(u32 v, u32 *wsum, u32 tid, u32 &total) {
  u32 const inc = wave_scan_incl(v);
  if ((tid & 63u) == 63u) wsum[tid >> 6] = inc;
  __syncthreads();
  u32 base = 0;
  for (u32 w = 0; w < (tid >> 6); w++) base += wsum[w];
  total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  return base + inc - v;
}

extern "C" __global__ __launch_bounds__(LDM_THREADS) void zh_ldm_index_kernel(const u8 *__restrict__ src, u64 size, u32 table_log, u64 *table,
                                                                              u64 *__restrict__ skey, u32 *__restrict__ sslot,
                                                                              u32 *__restrict__ scount) {
  __shared__ u32 stage[LDM_STAGE_LDS];
  __shared__ u32 wsum[4];
  u32 const c = blockIdx.x, tid = threadIdx.x;
  u64 const c0 = (u64)c * ZH_LDM_CELL;
  u64 const avail = size - c0;  // bytes from the cell's start to the frame's end (> 0)
  const u8 *const g = src + c0;
  // stage the cell and the 63 bytes after it (zero past the frame's end: those positions are
  // never hashed as positions, p + 64 <= size)
  for (u32 q = tid; q < LDM_STAGE_WORDS / 4u; q += LDM_THREADS) {
    uint4 v = make_uint4(0, 0, 0, 0);
    u64 const a = 16ull * q;
    if (a + 16u <= avail) {
      v = ld16(g + a);
    } else if (a < avail) {
      u32 w[4] = {0, 0, 0, 0};
      for (u32 k = 0; k < (u32)(avail - a); k++) w[k >> 2] |= (u32)g[a + k] << (8u * (k & 3u));
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    u32 const w0 = 4u * q;  // (4 dwords never straddle a pad: 32 is a multiple of 4)
    u32 const o = LDM_PAD(w0);
    stage[o] = v.x; stage[o + 1] = v.y; stage[o + 2] = v.z; stage[o + 3] = v.w;
  }
  __syncthreads();
  // positions of this lane: cell offsets [128 tid, 128 tid + 128), valid while p + 64 <= size
  u32 const j0 = LDM_RUN * tid;
  u32 const nvalid = avail >= ZH_LDM_HASH_BYTES ? (u32)min((u64)ZH_LDM_CELL, avail - ZH_LDM_HASH_BYTES + 1u) : 0u;  // valid cell offsets
  u32 const nmine = j0 < nvalid ? min(LDM_RUN, nvalid - j0) : 0u;
  u64 mlo = 0, mhi = 0;  // sample bits of the lane's positions, bit j = position j0 + j
  {
    u64 h = 0;
    u32 const base = LDM_PAD(j0 / 4u);  // (j0 / 4 is a multiple of 32: the lane's 48 dwords hold one pad, after the 32nd)
    for (u32 k = 0; k < 48u; k++) {
      u32 const w = stage[base + k + (k >> 5)];
#pragma unroll
      for (u32 b = 0; b < 4u; b++) {
        h = zh_ldm_roll(h, (w >> (8u * b)) & 255u);
        u32 const idx = 4u * k + b;  // bytes rolled in - 1
        if (idx >= ZH_LDM_HASH_BYTES - 1u && idx < ZH_LDM_HASH_BYTES - 1u + LDM_RUN) {
          u32 const j = idx - (ZH_LDM_HASH_BYTES - 1u);
          u64 const bit = (j < nmine && zh_ldm_is_sample(h)) ? 1ull : 0ull;
          mlo = (mlo >> 1) | (mhi << 63);
          mhi = (mhi >> 1) | (bit << 63);
        }
      }
    }
  }
  u32 const mine = (u32)__popcll(mlo) + (u32)__popcll(mhi);
  u32 total;
  u32 rank = block_scan_excl(mine, wsum, tid, total);
  if (tid == 0) scount[c] = min(total, ZH_LDM_CELL_SAMPLES);
  // second roll, for the lanes that own kept samples: emit them in position order
  if (mine && rank < ZH_LDM_CELL_SAMPLES) {
    u64 h = 0;
    u32 const base = LDM_PAD(j0 / 4u);
    u64 *const ck = skey + (size_t)c * ZH_LDM_CELL_SAMPLES;
    u32 *const cs = sslot + (size_t)c * ZH_LDM_CELL_SAMPLES;
    for (u32 k = 0; k < 48u && rank < ZH_LDM_CELL_SAMPLES; k++) {
      u32 const w = stage[base + k + (k >> 5)];
#pragma unroll
      for (u32 b = 0; b < 4u; b++) {
        h = zh_ldm_roll(h, (w >> (8u * b)) & 255u);
        u32 const idx = 4u * k + b;
        if (idx >= ZH_LDM_HASH_BYTES - 1u && idx < ZH_LDM_HASH_BYTES - 1u + LDM_RUN) {
          u32 const j = idx - (ZH_LDM_HASH_BYTES - 1u);
          bool const s = ((j < 64u ? mlo >> j : mhi >> (j - 64u)) & 1ull) != 0;
          if (s && rank < ZH_LDM_CELL_SAMPLES) {
            u64 const key = (c0 + j0 + j) << 32 | zh_ldm_tag(h);
            u32 const slot = zh_ldm_slot(h, table_log);
            ck[rank] = key;
            cs[rank] = slot;
            atomicMin((unsigned long long *)&table[slot], (unsigned long long)key);
            rank++;
          }
        }
      }
    }
  }
}

// per-byte equality of two 16-byte vectors as 16 bits
__device__ __forceinline__ u32 eq_bits4(u32 x) {  // bit k = byte k of x is zero
  u32 const z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);  // 0x80 per zero byte
  return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}
__device__ __forceinline__ u32 eq_mask16(uint4 a, uint4 b) {
  return eq_bits4(a.x ^ b.x) | eq_bits4(a.y ^ b.y) << 4 | eq_bits4(a.z ^ b.z) << 8 | eq_bits4(a.w ^ b.w) << 12;
}

struct LdmCellOut {
  ZhBlockDesc *descs;  // 3 per cell
  u8 *staging;         // ZH_STAGE_SLOT per slot
  u32 *blk_size;       // per slot
  ZhLdmRecord *rec;    // per cell
};

extern "C" __global__ __launch_bounds__(LDM_THREADS) void zh_ldm_cell_kernel(const u8 *__restrict__ src, u64 size, u32 ncells, u32 table_log,
                                                                             u32 max_dist, u32 flags, const u64 *__restrict__ table,
                                                                             const u64 *__restrict__ skey, const u32 *__restrict__ sslot,
                                                                             const u32 *__restrict__ scount, LdmCellOut out) {
  __shared__ u32 cand[ZH_LDM_CELL_SAMPLES];
  __shared__ u32 offs[ZH_LDM_CELL_OFFSETS + 1];  // [ZH_LDM_CELL_OFFSETS] = how many
  __shared__ __attribute__((aligned(16))) u16 masks[ZH_LDM_CELL / 16u];
  __shared__ u16 sufs[LDM_THREADS];
  __shared__ u32 ends[LDM_THREADS];
  __shared__ u32 wmax[4];
  __shared__ unsigned long long best_key;
  u32 const c = blockIdx.x, tid = threadIdx.x;
  u64 const c0 = (u64)c * ZH_LDM_CELL;
  u32 const cn = (u32)min((u64)ZH_LDM_CELL, size - c0);  // bytes of this cell
  u32 seg_start = 0, seg_len = 0, seg_dist = 0;          // (thread 0's copy decides)

  u32 const cnt = c ? scount[c] : 0u;
  if (cnt) {  // (block-uniform)
    // ---- candidates: kept samples whose slot holds an earlier position beyond K1's reach with the same 64 bytes
    for (u32 i = tid; i < ZH_LDM_CELL_SAMPLES; i += LDM_THREADS) {
      u32 d = 0;
      if (i < cnt) {
        u64 const key = skey[(size_t)c * ZH_LDM_CELL_SAMPLES + i];
        u64 const e = table[sslot[(size_t)c * ZH_LDM_CELL_SAMPLES + i]];
        u32 const p = (u32)(key >> 32), s = (u32)(e >> 32);
        if ((u32)e == (u32)key && s < p && p - s > ZH_LDM_MIN_DIST && p - s <= max_dist) {
          // (s + 64 <= p + 64 <= size: both were hashed as positions)
          bool same = true;
          for (u32 k = 0; k < ZH_LDM_HASH_BYTES; k += 16u) {
            uint4 const a = ld16(src + p + k), b = ld16(src + s + k);
            same &= (a.x == b.x) & (a.y == b.y) & (a.z == b.z) & (a.w == b.w);
          }
          if (same) d = p - s;
        }
      }
      cand[i] = d;
    }
    __syncthreads();
    // ---- the first ZH_LDM_CELL_OFFSETS distinct distances, by first appearance (wave 0)
    if (tid < 64u) {
      u32 k[ZH_LDM_CELL_OFFSETS] = {0, 0, 0, 0}, nk = 0;
      for (u32 ch = 0; ch < ZH_LDM_CELL_SAMPLES / 64u && nk < ZH_LDM_CELL_OFFSETS; ch++) {
        u32 const d = cand[ch * 64u + tid];
        while (nk < ZH_LDM_CELL_OFFSETS) {
          u64 const m = __ballot(d != 0 && d != k[0] && d != k[1] && d != k[2] && d != k[3]);
          if (!m) break;
          u32 const dn = (u32)__shfl((int)d, (int)__builtin_ctzll(m), 64);
          if (nk == 0) k[0] = dn; else if (nk == 1) k[1] = dn; else if (nk == 2) k[2] = dn; else k[3] = dn;
          nk++;
        }
      }
      if (tid == 0) { offs[0] = k[0]; offs[1] = k[1]; offs[2] = k[2]; offs[3] = k[3]; offs[ZH_LDM_CELL_OFFSETS] = nk; }
    }
    __syncthreads();
    u32 const noffs = offs[ZH_LDM_CELL_OFFSETS];
    // ---- per distance: the longest run of cell bytes equal to the bytes d back (lowest start on ties)
    for (u32 o = 0; o < noffs; o++) {
      u32 const d = offs[o];
      // cell offsets [lo, cn) are comparable (their source d back is inside the frame)
      u32 const lo = (u64)d > c0 ? (u32)((u64)d - c0) : 0u;  // (d <= p < c0 + cn, so lo < cn)
      if (tid == 0) best_key = 0;
      for (u32 q = tid; q < ZH_LDM_CELL / 16u; q += LDM_THREADS) {
        u32 const a = 16u * q;
        u32 m = 0;
        if (a >= lo && a + 16u <= cn) {
          m = eq_mask16(ld16(src + c0 + a), ld16(src + c0 + a - d));
        } else {
          for (u32 k = 0; k < 16u; k++) {
            u32 const i = a + k;
            if (i >= lo && i < cn && src[c0 + i] == src[c0 + i - d]) m |= 1u << k;
          }
        }
        masks[q] = (u16)m;
      }
      __syncthreads();
      // lane tid owns cell bytes [128 tid, 128 tid + 128): its equal bytes at both ends.  A run of
      // at least 128 bytes touches a lane boundary, so runs inside one lane are never looked at.
      uint4 const mv = ((const uint4 *)masks)[tid];
      u64 const ml = (u64)mv.y << 32 | mv.x, mh = (u64)mv.w << 32 | mv.z;
      bool const full = (ml & mh) == ~0ull;
      u32 const pre = full ? LDM_RUN : (ml == ~0ull ? 64u + (u32)__builtin_ctzll(~mh) : (u32)__builtin_ctzll(~ml));
      u32 const suf = full ? LDM_RUN : (mh == ~0ull ? 64u + (u32)__builtin_clzll(~ml) : (u32)__builtin_clzll(~mh));
      sufs[tid] = (u16)suf;
      // index + 1 of the last lane <= tid that is not all equal (0: none)
      u32 nf = wave_scan_max_incl(full ? 0u : tid + 1u);
      if ((tid & 63u) == 63u) wmax[tid >> 6] = nf;
      __syncthreads();
      for (u32 w = 0; w < (tid >> 6); w++) nf = max(nf, wmax[w]);
      // equal bytes ending at this lane's last byte
      u32 const e = nf == 0 ? LDM_RUN * (tid + 1u) : (u32)sufs[nf - 1u] + LDM_RUN * (tid - (nf - 1u));
      ends[tid] = e;
      __syncthreads();
      if (!full || tid == LDM_THREADS - 1u) {
        u32 const len = (tid ? ends[tid - 1u] : 0u) + pre;
        u32 const start = LDM_RUN * tid + pre - len;
        if (len) atomicMax(&best_key, (unsigned long long)len << 32 | (0xFFFFFFFFu - start));
      }
      __syncthreads();
      if (tid == 0) {
        u32 const len = (u32)(best_key >> 32);
        if (len > seg_len) {  // ties: the earlier distance stays
          seg_len = len;
          seg_start = 0xFFFFFFFFu - (u32)best_key;
          seg_dist = d;
        }
      }
      __syncthreads();  // (masks, sufs, ends, best_key are rewritten by the next distance)
    }
  }
  if (tid != 0) return;
  if (seg_len < ZH_LDM_MIN_SEG) seg_len = seg_start = seg_dist = 0;

  // ---- the cell's three slots
  bool const last_cell = c + 1u == ncells;
  u32 const n[3] = {seg_len ? seg_start : cn, 0u, seg_len ? cn - seg_start - seg_len : 0u};
  u32 const at[3] = {0u, seg_start, seg_start + seg_len};
  u32 const last_slot = !seg_len ? 0u : n[2] ? 2u : 1u;
  for (u32 k = 0; k < 3u; k++) {
    u32 const slot = 3u * c + k;
    ZhBlockDesc d;
    d.src = src + c0 + at[k];
    d.dst = out.staging + (size_t)slot * ZH_STAGE_SLOT;
    d.frame_size = size;
    d.n = n[k];
    d.item = 0;
    d.dst_cap = ZH_STAGE_SLOT;
    d.flags = 0;
    d.pre = nullptr;
    d.pre_n = 0;
    d.dict_id = 0;
    bool const ldm = k == 1u && seg_len;
    if (n[k] || ldm) d.flags = flags | (c == 0 ? ZH_F_FIRST : 0u) | (last_cell && k == last_slot ? ZH_F_LAST : 0u) | (ldm ? ZH_F_LDM : 0u);
    if (n[k] && c) {  // a later block of a history frame: the 32 KiB before it are staged in front
      d.pre = d.src - ZH_HIST_BLOCK;
      d.pre_n = ZH_HIST_BLOCK;
    }
    out.descs[slot] = d;
    out.blk_size[slot] = ldm ? zh_ldm_write_block(d.dst, seg_len, seg_dist, last_cell && last_slot == 1u) : 0u;
  }
  ZhLdmRecord r;
  r.seg_start = seg_len ? (u32)(c0 + seg_start) : 0u;
  r.seg_len = seg_len;
  r.distance = seg_dist;
  out.rec[c] = r;
}

namespace zh {

namespace {
struct LdmProf {
  std::mutex mu;
  bool on = false;
  std::vector<hipEvent_t> ev;  // pairs around the two kernels of each launch
};
LdmProf &ldm_prof() {
  static LdmProf p;
  return p;
}
}  // namespace

// HIP events around the finder's two kernels (tools/ldm_bench.py).  off: returns the summed
// milliseconds of the launches recorded since it was switched on
double ldm_profile(bool on) {
  LdmProf &p = ldm_prof();
  std::lock_guard<std::mutex> g(p.mu);
  double ms = 0;
  for (size_t i = 0; i + 1 < p.ev.size(); i += 2) {
    float t = 0;
    (void)hipEventSynchronize(p.ev[i + 1]);
    (void)hipEventElapsedTime(&t, p.ev[i], p.ev[i + 1]);
    ms += t;
    (void)hipEventDestroy(p.ev[i]);
    (void)hipEventDestroy(p.ev[i + 1]);
  }
  p.ev.clear();
  p.on = on;
  return ms;
}

// Index + split of one frame of ncells cells (size > ZH_BLOCK_MAX, size <= ZH_LDM_MAX_FRAME),
// stream-ordered; `flags` go on every active block (checksum, deep)
hipError_t ldm_launch(const u8 *src, u64 size, u32 ncells, u32 table_log, u32 max_dist, u32 flags, u64 *table, u64 *skey, u32 *sslot,
                      u32 *scount, ZhBlockDesc *descs, u8 *staging, u32 *blk_size, ZhLdmRecord *rec, hipStream_t stream) {
  // (profiling: the pair joins the list only once both events are recorded)
  bool prof;
  {
    std::lock_guard<std::mutex> g(ldm_prof().mu);
    prof = ldm_prof().on;
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (prof && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) {
    if (e0) (void)hipEventDestroy(e0);
    e0 = e1 = nullptr;
  }
  if (e0) (void)hipEventRecord(e0, stream);
  hipError_t const e = hipMemsetAsync(table, 0xFF, sizeof(u64) << table_log, stream);
  if (e != hipSuccess) {
    if (e0) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); }
    return e;
  }
  hipLaunchKernelGGL(zh_ldm_index_kernel, dim3(ncells), dim3(LDM_THREADS), 0, stream, src, size, table_log, table, skey, sslot, scount);
  LdmCellOut const out{descs, staging, blk_size, rec};
  hipLaunchKernelGGL(zh_ldm_cell_kernel, dim3(ncells), dim3(LDM_THREADS), 0, stream, src, size, ncells, table_log, max_dist, flags,
                     (const u64 *)table, (const u64 *)skey, (const u32 *)sslot, (const u32 *)scount, out);
  if (e0) {
    (void)hipEventRecord(e1, stream);
    std::lock_guard<std::mutex> g(ldm_prof().mu);
    ldm_prof().ev.push_back(e0);
    ldm_prof().ev.push_back(e1);
  }
  return hipGetLastError();
}

}  // namespace zh

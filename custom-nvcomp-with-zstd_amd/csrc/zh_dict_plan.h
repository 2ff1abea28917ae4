// zh_dict_plan.h — geometry of COVER training shared by the host trainer's check and the device
// trainer (zh_dict_train.hip).  Plain C++17, no HIP types: the names and the arithmetic are
// zh::cover_train's (zh_dict.cpp), so the two stay comparable line by line.
//
// The device formulation of one epoch step.  For the epoch [b, end) the candidate windows start
// at w in [b, wmax]; score(w) = sum of freq over the distinct buckets of [w, min(w + seg, end)).
// Position i counts in window w exactly when it is the first occurrence of its bucket in the
// window: w <= i < w + seg and the nearest earlier equal position p = i - prevdist[i] is < w.  So i
// adds freq[dm[i]] to the windows [lo, hi] of cover_range(): +f at diff[lo - b], -f at
// diff[hi + 1 - b], an inclusive prefix sum gives the scores, and the first maximum wins (the
// host's `score > best` is strict).  The host's partial windows while its window still grows are
// subsets of the first full window, so they never beat it and are no candidates of their own.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZH_PLAN_HD __host__ __device__
#else
#define ZH_PLAN_HD
#endif

namespace zh {

constexpr uint32_t kCoverHashBits = 20;  // buckets of d-mer ids
constexpr uint32_t kCoverNone = ~0u;     // dm of a position whose d-mer crosses its sample's end
constexpr uint32_t kCoverDefaultK = 1024, kCoverDefaultD = 8;
constexpr uint32_t kCoverMaxK = 65535;   // device trainer: prevdist is a u16

struct CoverPlan {
  uint32_t k, d;     // clamped: d in [4, 8], k >= 2 d
  uint64_t mask;     // the d low bytes of an 8-byte load
  size_t N, nd;      // corpus bytes; d-mer start positions N - d + 1
  size_t seg;        // d-mers per segment
  size_t epochs, esz;
  uint32_t max_zero;  // consecutive zero-score steps that end training
  bool empty;         // N < k or dict_size < d: the result is empty
};

ZH_PLAN_HD inline CoverPlan cover_plan(size_t N, size_t dict_size, uint32_t k, uint32_t d) {
  CoverPlan p;
  d = d < 4 ? 4 : d > 8 ? 8 : d;
  k = k < 2 * d ? 2 * d : k;
  p.k = k;
  p.d = d;
  p.mask = d >= 8 ? ~0ull : ((1ull << (8 * d)) - 1);
  p.N = N;
  p.empty = N < (size_t)k || dict_size < d;
  p.nd = N >= d ? N - d + 1 : 0;
  p.seg = k - d + 1;
  // epochs (libzstd COVER_computeEpochs): about dict_size / k / 4 of them, each >= 10 k
  p.epochs = dict_size / k / 4;
  if (p.epochs < 1) p.epochs = 1;
  p.esz = p.nd / p.epochs;
  if (p.esz < 10 * (size_t)k) {
    p.esz = p.nd < 10 * (size_t)k ? p.nd : 10 * (size_t)k;
    p.epochs = p.esz ? p.nd / p.esz : 1;
    if (p.epochs < 1) p.epochs = 1;
  }
  uint32_t const e8 = (uint32_t)(p.epochs >> 3 > 100 ? 100 : p.epochs >> 3);
  p.max_zero = e8 < 10 ? 10 : e8;
  return p;
}

// bucket of the d-mer whose 8-byte little-endian load is v
ZH_PLAN_HD inline uint32_t cover_hash(uint64_t v, uint64_t mask) {
  return (uint32_t)(((v & mask) * 0x9E3779B185EBCA87ull) >> (64 - kCoverHashBits));
}

struct CoverEpoch {
  size_t b, end;  // positions [b, end)
  size_t wmax;    // window starts [b, wmax]
};

ZH_PLAN_HD inline CoverEpoch cover_epoch(const CoverPlan &p, size_t e) {
  CoverEpoch ep;
  ep.b = e * p.esz;
  ep.end = ep.b + p.esz < p.nd ? ep.b + p.esz : p.nd;
  ep.wmax = ep.end - ep.b > p.seg ? ep.end - p.seg : ep.b;
  return ep;
}

// windows [lo, hi] that position i of the epoch scores in; false when there is none.
// prevdist: distance to the nearest earlier equal bucket within seg - 1 positions, 0 for none.
ZH_PLAN_HD inline bool cover_range(size_t i, uint32_t prevdist, size_t seg, const CoverEpoch &ep, size_t &lo, size_t &hi) {
  lo = prevdist ? i - prevdist + 1 : 0;
  size_t const ws = i + 1 >= seg ? i + 1 - seg : 0;
  if (lo < ws) lo = ws;
  if (lo < ep.b) lo = ep.b;
  hi = i < ep.wmax ? i : ep.wmax;
  return lo <= hi;
}

// bytes a committed segment [sb, se) gives the dictionary, whose free space is `tail`
ZH_PLAN_HD inline size_t cover_commit_bytes(size_t sb, size_t se, uint32_t d, size_t tail) {
  size_t const bytes = se - sb + d - 1;
  return bytes < tail ? bytes : tail;
}

// ---- device trainer: temp buffer -------------------------------------------------------------
constexpr size_t kCoverScanTile = 2048;  // diff entries per scan workgroup

struct CoverCtl {  // the trainer's state in device memory
  uint32_t tail;      // free bytes at the head of dict
  uint32_t zero_run;
  uint32_t epoch;     // cursor: the epoch of the next step
  uint32_t done;
};

// ---- groups: one dictionary per run of consecutive samples ------------------------------------
// The samples of all groups lie back to back; group g owns the positions [base, base + plan.N) of
// the concatenation.  Epochs, windows and commits are cover_epoch / cover_range /
// cover_commit_bytes in group-local positions; only the loads of dm, prev and the corpus add base,
// and the look-back of a position stops at its group's first one (cover_lookback).  One
// dictionary from all samples is the call with one group.
constexpr size_t kCoverGroupsInFlight = 64;  // slots of per-group state; more groups run as successive waves
constexpr size_t kCoverMaxGroups = 4096;     // what a dictionary set holds

struct CoverGroup {
  CoverPlan plan;  // cover_plan(the group's own bytes, dict_size, k, d)
  uint64_t base;   // its first position in the concatenation
  uint32_t s0, s1;  // its samples [s0, s1)
  uint32_t slot;    // its slot of the per-group temp arrays: g % kCoverGroupsInFlight
  uint32_t ntiles;  // scan tiles of one of its epochs (its windows plus the entry after the last one)
};

ZH_PLAN_HD inline size_t cover_scan_tiles(const CoverPlan &p) { return (p.esz + 1 + kCoverScanTile - 1) / kCoverScanTile; }

// records of the ng groups of counts[g] consecutive samples each (the counts sum to the number
// of sizes); returns the bytes of all samples
inline uint64_t cover_groups(const size_t *sizes, const size_t *counts, size_t ng, size_t dict_size, uint32_t k, uint32_t d, CoverGroup *out) {
  uint64_t base = 0;
  size_t s = 0;
  for (size_t g = 0; g < ng; g++) {
    uint64_t n = 0;
    for (size_t j = 0; j < counts[g]; j++) n += sizes[s + j];
    CoverGroup &G = out[g];
    G.plan = cover_plan((size_t)n, dict_size, k, d);
    G.base = base;
    G.s0 = (uint32_t)s;
    G.s1 = (uint32_t)(s + counts[g]);
    G.slot = (uint32_t)(g % kCoverGroupsInFlight);
    G.ntiles = (uint32_t)cover_scan_tiles(G.plan);
    s += counts[g];
    base += n;
  }
  return base;
}

// farthest look-back of the group-local position `local`: inside the segment and inside the group
ZH_PLAN_HD inline uint32_t cover_lookback(size_t seg, uint64_t local) { return (uint32_t)(local < seg - 1 ? local : seg - 1); }

// waves of at most kCoverGroupsInFlight groups: wave w holds the groups [w * 64, min(ng, w * 64 + 64))
ZH_PLAN_HD inline size_t cover_waves(size_t ng) { return (ng + kCoverGroupsInFlight - 1) / kCoverGroupsInFlight; }

struct CoverTempLayout {
  // byte offsets, each a multiple of 256.  groups, ends, dm and prev belong to the call; ctl, freq,
  // diff, tsum, tbest and dict hold `slots` slots of the strides below, the offset being slot 0's
  size_t groups, ends, dm, prev, ctl, freq, diff, tsum, tbest, dict;
  size_t slots;   // groups in flight
  size_t ntiles;  // scan tiles of one epoch of the largest group
  size_t freq_stride, diff_stride, tsum_stride, tbest_stride, dict_stride;  // bytes (ctl: sizeof(CoverCtl))
  size_t total;
};

ZH_PLAN_HD inline size_t cover_align256(size_t v) { return (v + 255) & ~(size_t)255; }

// total_bytes: the bytes of all samples; max_ntiles: the largest cover_scan_tiles of the groups
ZH_PLAN_HD inline CoverTempLayout cover_temp_layout(size_t total_bytes, size_t num_samples, size_t num_groups, size_t max_ntiles,
                                                    size_t dict_size) {
  CoverTempLayout L;
  size_t o = 0;
  L.slots = num_groups < kCoverGroupsInFlight ? num_groups : kCoverGroupsInFlight;
  L.ntiles = max_ntiles;
  L.groups = o, o += cover_align256(num_groups * sizeof(CoverGroup));
  L.ends = o, o += cover_align256(num_samples * 4);
  L.dm = o, o += cover_align256(total_bytes * 4);
  L.prev = o, o += cover_align256(total_bytes * 2);
  L.ctl = o, o += cover_align256(L.slots * sizeof(CoverCtl));
  L.freq_stride = (size_t)4 << kCoverHashBits;
  L.freq = o, o += L.slots * L.freq_stride;
  L.diff_stride = L.ntiles * kCoverScanTile * 8;
  L.diff = o, o += L.slots * L.diff_stride;
  L.tsum_stride = cover_align256(L.ntiles * 8);
  L.tsum = o, o += L.slots * L.tsum_stride;
  L.tbest_stride = cover_align256(L.ntiles * 16);
  L.tbest = o, o += L.slots * L.tbest_stride;
  L.dict_stride = cover_align256(dict_size);
  L.dict = o, o += L.slots * L.dict_stride;
  L.total = o + 256;  // the caller's pointer is aligned up to 256
  return L;
}

// what cuda_zstd_train_dictionaries_device_get_temp_size reports: enough for every d of [4, 8]
inline size_t cover_temp_bytes(const size_t *sizes, size_t num_samples, const size_t *counts, size_t num_groups, size_t dict_size, uint32_t k) {
  size_t m = 0;
  for (uint32_t d = 4; d <= 8; d++) {
    size_t s = 0, nt = 0;
    uint64_t total = 0;
    for (size_t g = 0; g < num_groups; g++) {
      uint64_t n = 0;
      for (size_t j = 0; j < counts[g]; j++) n += sizes[s + j];
      s += counts[g];
      total += n;
      size_t const t = cover_scan_tiles(cover_plan((size_t)n, dict_size, k ? k : kCoverDefaultK, d));
      if (t > nt) nt = t;
    }
    size_t const t = cover_temp_layout((size_t)total, num_samples, num_groups, nt, dict_size).total;
    if (t > m) m = t;
  }
  return m;
}

// what cuda_zstd_train_dictionary_device_get_temp_size reports: the call with one group
inline size_t cover_temp_bytes(size_t total_sample_bytes, size_t num_samples, size_t dict_size, uint32_t k) {
  size_t m = 0;
  for (uint32_t d = 4; d <= 8; d++) {
    size_t const nt = cover_scan_tiles(cover_plan(total_sample_bytes, dict_size, k ? k : kCoverDefaultK, d));
    size_t const t = cover_temp_layout(total_sample_bytes, num_samples, 1, nt, dict_size).total;
    if (t > m) m = t;
  }
  return m;
}

}  // namespace zh

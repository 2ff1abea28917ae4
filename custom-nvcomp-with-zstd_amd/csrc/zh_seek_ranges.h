// zh_seek_ranges.h — the arithmetic of a batched range read of a seekable stream, shared by the
// device kernels (zh_seek.hip), the host (zh_host_seek.cpp) and a stand-alone host check
// (tests/cpp/seek_ranges_check.cpp).  Plain integer code, no HIP calls.
//
// The scanned table is two arrays: ld[i], the content offset of entry i inside its tile of
// ZH_SEEK_TILE entries, and tbd[t], the content offset of tile t.  start(i) = tbd[i / TILE] +
// ld[i] never decreases; an entry of size 0 (an empty frame, a skippable frame listed in the
// table) shares its start with the next entry.
//   cover    : the entry that holds content byte pos — a two-level binary search, tiles first
//   next_seg : the walk of a content interval over the entries with content that hold it
//   layout   : where a batched read keeps its arrays in the temp buffer
#pragma once
#include "zh_seek_format.h"

#define ZH_SEEK_TILE 1024u    // entries per scan tile (zh_seek.hip's SK_TILE)
#define ZH_SEEK_PIECE 16384u  // content bytes per scatter workgroup

// Marks of a range that covers no entry, in its `first` slot (`last` is then unused)
#define ZH_SEEK_RANGE_EMPTY 0xFFFFFFFEu
#define ZH_SEEK_RANGE_INVALID 0xFFFFFFFFu
#define ZH_SEEK_NO_JOB 0xFFFFFFFFu

struct ZhSeekIndex {
  const uint64_t *ld;   // n tile-local exclusive sums of Decompressed_Size
  const uint64_t *tbd;  // ceil(n / TILE) exclusive tile bases
  uint64_t n;           // entries
  uint64_t total;       // bytes of content
};

ZH_SEEK_HD uint64_t zh_seek_start(const ZhSeekIndex &x, uint64_t i) {  // i <= n
  return i < x.n ? x.tbd[i / ZH_SEEK_TILE] + x.ld[i] : x.total;
}

// The entry that holds content byte pos < total: the last i with start(i) <= pos.  It has
// content: an entry of size 0 at start(i) <= pos is followed by one with the same start.
ZH_SEEK_HD uint64_t zh_seek_cover(const ZhSeekIndex &x, uint64_t pos) {
  uint64_t lo = 0, hi = (x.n + ZH_SEEK_TILE - 1) / ZH_SEEK_TILE;  // tbd[lo] <= pos (tbd[0] = 0); tbd[hi] > pos or hi is the end
  while (hi - lo > 1) {
    uint64_t const mid = lo + (hi - lo) / 2;
    if (x.tbd[mid] <= pos) lo = mid;
    else hi = mid;
  }
  uint64_t const t0 = lo * ZH_SEEK_TILE, rel = pos - x.tbd[lo];
  lo = 0;
  hi = x.n - t0 < ZH_SEEK_TILE ? x.n - t0 : ZH_SEEK_TILE;  // ld[t0] = 0 <= rel
  while (hi - lo > 1) {
    uint64_t const mid = lo + (hi - lo) / 2;
    if (x.ld[t0 + mid] <= rel) lo = mid;
    else hi = mid;
  }
  return t0 + lo;
}

// Whether a range lies inside the content and under the call's bound
ZH_SEEK_HD bool zh_seek_range_ok(uint64_t offset, uint64_t length, uint64_t total, uint64_t max_length) {
  return length <= max_length && offset <= total && length <= total - offset;
}

struct ZhSeekSeg {
  uint64_t frame;     // entry index
  uint64_t in_frame;  // first byte inside the frame's content
  uint64_t pos;       // the same byte's content offset
  uint64_t len;       // > 0
};

// One step of the walk over [*pos, end), end <= total: *i is the entry to look at (start with
// zh_seek_cover(*pos)).  Gives the next segment and moves *i and *pos past it; false at the end.
ZH_SEEK_HD bool zh_seek_next_seg(const ZhSeekIndex &x, uint64_t *i, uint64_t *pos, uint64_t end, ZhSeekSeg *s) {
  while (*pos < end) {
    uint64_t const a = zh_seek_start(x, *i), b = zh_seek_start(x, *i + 1);
    if (b <= *pos) {  // an entry of size 0 (a <= *pos always holds)
      ++*i;
      continue;
    }
    uint64_t const stop = b < end ? b : end;
    s->frame = *i;
    s->in_frame = *pos - a;
    s->pos = *pos;
    s->len = stop - *pos;
    *pos = stop;
    ++*i;
    return true;
  }
  return false;
}

// Temp buffer of a batched read, as offsets from its 256-aligned base: the fixed part of a read
// (sized by the table's N: control block, the scanned columns, the decoder's job arrays), one
// bit per entry (touched by a range), the job of every entry, the first and last entry of every
// range, one staging slot of align256(max_d) bytes per decode job, the decoder's workspace.
struct ZhSeekRangesLayout {
  size_t bitmap, bitmap_bytes, job_of_frame, first, last, staging, slot, dec, total;
};

ZH_SEEK_HD size_t zh_seek_align256(size_t v) { return (v + 255) & ~(size_t)255; }

ZH_SEEK_HD ZhSeekRangesLayout zh_seek_ranges_layout(size_t fixed_bytes, size_t n, size_t num_ranges, size_t jobs, size_t max_d, size_t dec_bytes) {
  ZhSeekRangesLayout L;
  size_t o = zh_seek_align256(fixed_bytes);
  L.bitmap_bytes = (n + 31) / 32 * 4;
  L.bitmap = o; o = zh_seek_align256(o + L.bitmap_bytes);
  L.job_of_frame = o; o = zh_seek_align256(o + n * 4);
  L.first = o; o = zh_seek_align256(o + num_ranges * 4);
  L.last = o; o = zh_seek_align256(o + num_ranges * 4);
  L.slot = zh_seek_align256(max_d ? max_d : 1);
  L.staging = o; o += jobs * L.slot;
  L.dec = o; o = zh_seek_align256(o + dec_bytes);
  L.total = o + 256;  // slack for base alignment
  return L;
}

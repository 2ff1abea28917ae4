// zh_frames.h — one frame's extent in a buffer of concatenated Zstandard frames (RFC 8878 §3.1),
// shared by the frame-index kernels (zh_frames.hip) and the host.  Plain integer code, no HIP calls.
//
// zh_frame_span restates, for extents only, what the decoder's walker does (zh_decode.hip):
// frame_header's checks and the `stated` branch of decode_body's Size pass.  It accepts and
// rejects the same bytes; it makes no dictionary check (an extent does not depend on one) and it
// never reads outside [p, p + n).  tests/test_frames_span.py and tests/test_gpu_frames_index.py
// pin the two together.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZH_FRAMES_HD __host__ __device__ inline
#else
#define ZH_FRAMES_HD inline
#endif

#define ZH_FRAMES_MAGIC 0xFD2FB528u
#define ZH_FRAMES_SKIP_MAGIC 0x184D2A50u  // .. 0x184D2A5F
#define ZH_FRAMES_BLOCK_MAX (128u * 1024u)
#define ZH_FRAMES_WINDOWLOG_MAX 30u
#define ZH_FRAMES_NO_FCS (~0ull)

// The scan kernels' tile: 256 lanes x 16 bytes of the stream per workgroup step.  With a
// 16-byte-aligned stream pointer, tile k covers the offsets [k * ZH_FRAMES_TILE, (k + 1) *
// ZH_FRAMES_TILE) and lane l of it the 16 bytes at l * ZH_FRAMES_LANE_BYTES (an unaligned
// pointer shifts the tiles down by its low four bits).
#define ZH_FRAMES_LANE_BYTES 16u
#define ZH_FRAMES_TILE 4096u
// Candidates the index's temp buffer holds for a call's max_frames; a stream with more of them
// (frames nested in raw blocks or skippable payloads) is indexed by the serial walker.
#define ZH_FRAMES_CANDIDATES(max_frames) (2ull * (max_frames) + 1024ull)

// The walker's statuses (the decoder's ST_* values), and the nvcomp-style codes the C ABI returns
enum : uint32_t { ZH_FRAMES_OK = 0, ZH_FRAMES_BAD_MAGIC = 5, ZH_FRAMES_CORRUPT = 6 };
ZH_FRAMES_HD uint32_t zh_frames_code(uint32_t status) {  // zh_decode.hip to_nvcomp
  return status == ZH_FRAMES_OK ? 0u : status == ZH_FRAMES_CORRUPT ? 6u : 1u;
}

struct ZhFrameSpan {
  uint64_t size;       // bytes of the whole frame, header to checksum
  uint64_t fcs;        // Frame_Content_Size; ZH_FRAMES_NO_FCS: absent (a skippable frame: 0)
  uint32_t skippable;  // 1: a skippable frame
};

ZH_FRAMES_HD bool zh_frames_is_skip_magic(uint32_t m) { return (m & 0xFFFFFFF0u) == ZH_FRAMES_SKIP_MAGIC; }
ZH_FRAMES_HD bool zh_frames_is_magic(uint32_t m) { return m == ZH_FRAMES_MAGIC || zh_frames_is_skip_magic(m); }

ZH_FRAMES_HD uint32_t zh_frames_ld32(const uint8_t *p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// The frame that starts at p, n bytes before the buffer's end (first: the buffer starts here).
// -> ZH_FRAMES_OK and *s, or the walker's error for these bytes.
ZH_FRAMES_HD uint32_t zh_frame_span(const uint8_t *p, uint64_t n, bool first, ZhFrameSpan *s) {
  if (n < 4) return ZH_FRAMES_CORRUPT;
  uint32_t const magic = zh_frames_ld32(p);
  if (zh_frames_is_skip_magic(magic)) {
    if (n < 8) return ZH_FRAMES_CORRUPT;
    s->size = 8ull + zh_frames_ld32(p + 4);
    s->fcs = 0;
    s->skippable = 1;
    return s->size > n ? ZH_FRAMES_CORRUPT : ZH_FRAMES_OK;
  }
  if (magic != ZH_FRAMES_MAGIC) return first ? ZH_FRAMES_BAD_MAGIC : ZH_FRAMES_CORRUPT;
  if (n < 5) return ZH_FRAMES_CORRUPT;
  // ---- frame header (RFC 8878 §3.1.1.1)
  uint32_t const fhd = p[4];
  uint32_t const fcsf = fhd >> 6, single = (fhd >> 5) & 1u, didf = fhd & 3u;
  if (fhd & 8u) return ZH_FRAMES_CORRUPT;  // reserved bit
  uint32_t const didn = didf == 3 ? 4u : didf;
  uint32_t const fcsn = fcsf == 0 ? single : 1u << fcsf;
  uint64_t ip = 5ull + (single ? 0u : 1u) + didn + fcsn;
  if (n < ip) return ZH_FRAMES_CORRUPT;
  const uint8_t *q = p + 5;
  if (!single) {
    if (10u + (*q++ >> 3) > ZH_FRAMES_WINDOWLOG_MAX) return ZH_FRAMES_CORRUPT;
  }
  q += didn;
  uint64_t fcs = ZH_FRAMES_NO_FCS;
  if (fcsn == 1) fcs = q[0];
  else if (fcsn == 2) fcs = ((uint64_t)q[0] | (uint64_t)q[1] << 8) + 256ull;
  else if (fcsn == 4) fcs = zh_frames_ld32(q);
  else if (fcsn == 8) fcs = (uint64_t)zh_frames_ld32(q) | (uint64_t)zh_frames_ld32(q + 4) << 32;
  // ---- blocks (RFC 8878 §3.1.1.2): the extent alone
  for (;;) {
    if (n - ip < 3) return ZH_FRAMES_CORRUPT;
    uint32_t const bh = (uint32_t)p[ip] | (uint32_t)p[ip + 1] << 8 | (uint32_t)p[ip + 2] << 16;
    uint32_t const last = bh & 1u, bt = (bh >> 1) & 3u, bsz = bh >> 3;
    ip += 3;
    uint64_t const body = bt == 1 ? 1u : bsz;
    if (bt == 3 || (bt == 2 && bsz >= ZH_FRAMES_BLOCK_MAX) || n - ip < body) return ZH_FRAMES_CORRUPT;
    ip += body;
    if (last) break;
  }
  if (fhd & 4u) {  // Content_Checksum
    if (n - ip < 4) return ZH_FRAMES_CORRUPT;
    ip += 4;
  }
  s->size = ip;
  s->fcs = fcs;
  s->skippable = 0;
  return ZH_FRAMES_OK;
}

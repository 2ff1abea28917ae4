// zh_ldm.h — long-distance matching: the definitions shared by the finder kernels (zh_ldm.hip),
// the host (zh_host.cpp) and the CPU checks (tests/cpp/ldm_block_check.cpp, tests/zh_ldm_model.py):
// the sample hash, the table geometry and the writer of a one-sequence block.  Host + device, no
// HIP header needed, so a plain C++ compiler can build it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ZH_LDM_HD __host__ __device__ inline
#else
#define ZH_LDM_HD inline
#endif

#define ZH_LDM_HASH_BYTES 64u    // bytes a position's hash covers
#define ZH_LDM_RATE_LOG 7u       // one position in 2^7 is a sample
#define ZH_LDM_CELL 32768u       // the frame's 32 KiB grid (= ZH_HIST_BLOCK)
#define ZH_LDM_CELL_SAMPLES 512u // samples kept per cell (the first ones in position order)
#define ZH_LDM_CELL_OFFSETS 4u   // distinct candidate distances scanned per cell
// Shortest run worth a block of its own.  Tried 256 and 4096: the same frame, byte count for byte
// count, on the text + JSON corpora followed by a shuffled copy of their own 4-16 KiB pieces (a
// cell takes its one longest run, and that was never under 4 KiB there).
#define ZH_LDM_MIN_SEG 1024u
#define ZH_LDM_MIN_DIST 32768u   // exclusive: K1 reaches 32 KiB back itself
// The predefined offset table ends at code 28: offset value = distance + 3 < 2^29
#define ZH_LDM_MAX_DIST ((1u << 29) - 4u)
#define ZH_LDM_MAX_FRAME 0xFFFFFFFFull  // positions are 32-bit (table entry = position << 32 | tag)
#define ZH_LDM_BLOCK_MAX 16u     // bytes of the largest LDM block (3 header + 3 + 8 of bit stream)

// ---------------------------------------------------------------------------------------------
// Hash: h <- (h << 1) + g(byte) over the 64 bytes at p, mod 2^64.  A byte's term has left the 64
// bits after 64 steps, so rolling one byte forward is the same step and a position's hash depends
// on exactly its 64 bytes.  g is arithmetic (24-bit multiplies, full rate on gfx950), no table.
ZH_LDM_HD uint32_t zh_ldm_mul24(uint32_t a, uint32_t b) { return (uint32_t)((uint64_t)(a & 0xFFFFFFu) * (uint64_t)(b & 0xFFFFFFu)); }
ZH_LDM_HD uint64_t zh_ldm_g(uint32_t byte) {
  uint32_t const x = (byte + 1u) * 0x9E3779u;  // < 2^32
  uint32_t const y = (x ^ (x >> 13)) & 0xFFFFFFu;
  return (uint64_t)zh_ldm_mul24(y, 0x85EBCAu) << 32 | zh_ldm_mul24(y ^ 0xC2B2AEu, 0x27D4EBu);
}
ZH_LDM_HD uint64_t zh_ldm_roll(uint64_t h, uint32_t byte) { return (h << 1) + zh_ldm_g(byte); }
ZH_LDM_HD uint64_t zh_ldm_hash(const uint8_t *p) {
  uint64_t h = 0;
  for (uint32_t i = 0; i < ZH_LDM_HASH_BYTES; i++) h = zh_ldm_roll(h, p[i]);
  return h;
}
// The low bits of h depend on the last bytes only: predicate, slot and tag come from the top bits
// of products that every bit of h reaches.
ZH_LDM_HD bool zh_ldm_is_sample(uint64_t h) {
  uint32_t const m = (uint32_t)(h >> 32) * 0x9E3779B1u + (uint32_t)h * 0x85EBCA77u;
  return (m >> (32u - ZH_LDM_RATE_LOG)) == (1u << ZH_LDM_RATE_LOG) - 1u;
}
ZH_LDM_HD uint32_t zh_ldm_slot(uint64_t h, uint32_t table_log) { return (uint32_t)((h * 0x9E3779B185EBCA87ull) >> (64u - table_log)); }
ZH_LDM_HD uint32_t zh_ldm_tag(uint64_t h) { return (uint32_t)(((h ^ (h >> 32)) * 0xC2B2AE3D27D4EB4Full) >> 32); }

// Table slots = 2^min(hash_log, max(10, ceil_log2(frame bytes) - ZH_LDM_RATE_LOG + 1)), hash_log >= 10
ZH_LDM_HD uint32_t zh_ldm_table_log(uint64_t frame_bytes, uint32_t hash_log) {
  uint32_t cl = 0;
  while (cl < 63u && (1ull << cl) < frame_bytes) cl++;
  uint32_t want = cl + 1u > ZH_LDM_RATE_LOG + 10u ? cl + 1u - ZH_LDM_RATE_LOG : 10u;
  if (hash_log < 10u) hash_log = 10u;
  if (hash_log > 30u) hash_log = 30u;
  return want < hash_log ? want : hash_log;
}

// Largest usable distance for a frame compressed with this window
ZH_LDM_HD uint32_t zh_ldm_max_dist(uint32_t window_log) {
  return window_log >= 29u ? ZH_LDM_MAX_DIST : (1u << window_log);
}

// ---------------------------------------------------------------------------------------------
// One-sequence block (RFC 8878 3.1.1.3): empty raw literals section, one sequence with literal
// length 0, match length ml and offset value dist + 3, all three tables predefined.

// Lowest state of the predefined table (normalised counts norm[0..nsym), 2^log states) that
// decodes to symbol sym: the table is spread as the RFC says (4.1.1).  A single sequence reads its
// three initial states and never steps them, so any state carrying the symbol serves.
ZH_LDM_HD uint32_t zh_ldm_fse_state(const int8_t *norm, uint32_t nsym, uint32_t log, uint32_t sym) {
  uint32_t const size = 1u << log, mask = size - 1u, step = (size >> 1) + (size >> 3) + 3u;
  uint32_t high = size - 1u, best = size;
  for (uint32_t s = 0; s < nsym; s++)
    if (norm[s] == -1) {
      if (s == sym) best = high;
      high--;
    }
  uint32_t pos = 0;
  for (uint32_t s = 0; s < nsym; s++) {
    if (norm[s] <= 0) continue;
    for (int32_t i = 0; i < norm[s]; i++) {
      if (s == sym && pos < best) best = pos;
      pos = (pos + step) & mask;
      while (pos > high) pos = (pos + step) & mask;
    }
  }
  return best;
}

// Writes the block (header included) for 3 <= ml <= 65538 + 65535 and 1 <= dist <= ZH_LDM_MAX_DIST;
// returns its size (<= ZH_LDM_BLOCK_MAX).  Byte stores only.
ZH_LDM_HD uint32_t zh_ldm_write_block(uint8_t *out, uint32_t ml, uint32_t dist, uint32_t last) {
  const int8_t nLL[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
  const int8_t nOF[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
  const int8_t nML[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                          1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
  const uint8_t mlBase[11] = {35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99}, mlBits[11] = {1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5};  // codes 32..42
  // offset: code = floor(log2(value)), that many extra bits
  uint32_t const ofv = dist + 3u;
  uint32_t ofc = 0;
  while ((ofv >> (ofc + 1u)) != 0u) ofc++;
  uint32_t const ofx = ofv - (1u << ofc);
  // match length code, extra bits
  uint32_t mlc, mlx, mln;
  if (ml < 35u) { mlc = ml - 3u; mlx = 0; mln = 0; }
  else if (ml < 131u) {
    mlc = 42u;
    while (mlBase[mlc - 32u] > ml) mlc--;
    mlx = ml - mlBase[mlc - 32u];
    mln = mlBits[mlc - 32u];
  } else {
    uint32_t const v = ml - 3u;
    mln = 0;
    while ((v >> (mln + 1u)) != 0u) mln++;
    mlc = mln + 36u;
    mlx = v - (1u << mln);
  }
  // bit stream, first bit written = last bit read: ML extra, OF extra, then the states ML, OF, LL
  // (the decoder reads LL, OF, ML states, then OF, ML, LL extra bits), then the end mark
  uint64_t acc = 0;
  uint32_t nb = 0;
  acc |= (uint64_t)mlx << nb; nb += mln;
  acc |= (uint64_t)ofx << nb; nb += ofc;
  acc |= (uint64_t)zh_ldm_fse_state(nML, 53, 6, mlc) << nb; nb += 6;
  acc |= (uint64_t)zh_ldm_fse_state(nOF, 29, 5, ofc) << nb; nb += 5;
  acc |= (uint64_t)zh_ldm_fse_state(nLL, 36, 6, 0) << nb; nb += 6;
  acc |= 1ull << nb; nb += 1;
  uint32_t const nbytes = (nb + 7u) >> 3, body = 3u + nbytes;
  uint32_t const hdr = (last & 1u) | (2u << 1) | (body << 3);
  out[0] = (uint8_t)hdr; out[1] = (uint8_t)(hdr >> 8); out[2] = (uint8_t)(hdr >> 16);
  out[3] = 0;  // literals section: raw, 0 bytes
  out[4] = 1;  // one sequence
  out[5] = 0;  // LL, OF, ML tables predefined
  for (uint32_t k = 0; k < nbytes; k++) out[6 + k] = (uint8_t)(acc >> (8u * k));
  return 3u + body;
}

// What the finder reports per cell (cuda_zstd_hip_ldm_plan): seg_len 0 = the cell is not split
struct ZhLdmRecord {
  uint32_t seg_start;  // frame position of the run's first byte
  uint32_t seg_len;
  uint32_t distance;
};

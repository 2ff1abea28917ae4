// zh_dict_entropy.h — host parser of a formatted dictionary's entropy section (RFC 8878 §5) into
// the encoder's blob (ZhDictEnt, zh_dict_ent.h): the Huffman code of the literals, the three FSE
// encoding tables in the entropy kernel's own layout, a fixed-point bit cost per symbol and the
// three repcodes.  Header only and HIP free: zh_host.cpp builds the blob once per dictionary at
// load, tests/cpp/dict_entropy_check.cpp runs the parser under the sanitizers.
#pragma once
#include <stddef.h>
#include <string.h>

#include "zh_dict_ent.h"

namespace zh {
namespace dent {
typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;
typedef int16_t s16;
typedef int32_t s32;

inline u32 highbit(u32 v) {
  u32 r = 0;
  while (v >>= 1) r++;
  return r;
}

// 32 bits starting at bit `bitpos` (LSB first), zeros past `avail` bytes
inline u32 fwd32(const u8 *p, size_t avail, size_t bitpos) {
  size_t const b = bitpos >> 3;
  u64 v = 0;
  for (size_t i = 0; i < 5; i++)
    if (b + i < avail) v |= (u64)p[b + i] << (8 * i);
  return (u32)(v >> (bitpos & 7));
}

// FSE_readNCount (RFC 8878 §4.1.1): normalised counts (-1 = "less than one") of symbols
// [0, *maxSV], the table log; returns the bytes used, 0 if malformed.  norm holds maxSVin + 1.
inline size_t read_ncount(const u8 *p, size_t avail, u32 maxSVin, u32 maxLog, s16 *norm, u32 *maxSV, u32 *tableLog) {
  if (!avail) return 0;
  u32 nb = (fwd32(p, avail, 0) & 15u) + 5u;
  if (nb > maxLog) return 0;
  *tableLog = nb;
  size_t bp = 4;
  int rem = (1 << nb) + 1, thr = 1 << nb;
  nb++;
  u32 sym = 0;
  bool prev0 = false;
  for (u32 s = 0; s <= maxSVin; s++) norm[s] = 0;
  while (rem > 1 && sym <= maxSVin) {
    if (prev0) {
      u32 n0 = sym, r;
      do {
        r = fwd32(p, avail, bp) & 3u;
        bp += 2;
        n0 += r;
      } while (r == 3 && bp < 8 * avail + 32);
      if (n0 > maxSVin) return 0;
      sym = n0;
    }
    u32 const bs = fwd32(p, avail, bp);
    int const mx = (2 * thr - 1) - rem;
    int c;
    if ((int)(bs & (u32)(thr - 1)) < mx) {
      c = (int)(bs & (u32)(thr - 1));
      bp += nb - 1;
    } else {
      c = (int)(bs & (u32)(2 * thr - 1));
      if (c >= thr) c -= mx;
      bp += nb;
    }
    c--;
    rem -= c < 0 ? -c : c;
    norm[sym++] = (s16)c;
    prev0 = c == 0;
    while (rem < thr) {
      nb--;
      thr >>= 1;
    }
  }
  if (rem != 1 || sym == 0) return 0;
  *maxSV = sym - 1;
  size_t const used = (bp + 7) >> 3;
  return used <= avail ? used : 0;
}

// FSE_buildCTable (the entropy kernel's fse_build_ctable_par serially): st holds 1 << tableLog
// states, sym (dNb, dFS) pairs of symbols [0, nsym); symbols past maxSV get the zero-count form
inline void build_ctable(u16 *st, u32 *sym2, u32 nsym, const s16 *norm, u32 maxSV, u32 tableLog) {
  u32 const T = 1u << tableLog, mask = T - 1, step = (T >> 1) + (T >> 3) + 3;
  u8 tsym[512];
  u32 cumul[66];
  u32 high = T - 1;
  cumul[0] = 0;
  for (u32 s = 0; s <= maxSV; s++) {
    if (norm[s] == -1) {
      cumul[s + 1] = cumul[s] + 1;
      tsym[high--] = (u8)s;
    } else {
      cumul[s + 1] = cumul[s] + (u32)norm[s];
    }
  }
  u32 pos = 0;
  for (u32 s = 0; s <= maxSV; s++)
    for (int i = 0; i < norm[s]; i++) {
      tsym[pos] = (u8)s;
      pos = (pos + step) & mask;
      while (pos > high) pos = (pos + step) & mask;
    }
  u32 next[66];
  memcpy(next, cumul, sizeof(next));
  for (u32 u = 0; u < T; u++) st[next[tsym[u]]++] = (u16)(T + u);
  for (u32 s = 0; s < nsym; s++) {
    int const nv = s <= maxSV ? norm[s] : 0;
    u32 dnb;
    s32 dfs;
    if (nv == 0) {
      dnb = ((tableLog + 1) << 16) - T;
      dfs = 0;
    } else if (nv == -1 || nv == 1) {
      dnb = (tableLog << 16) - T;
      dfs = (s32)cumul[s] - 1;
    } else {
      u32 const mbo = tableLog - highbit((u32)nv - 1);
      dnb = (mbo << 16) - ((u32)nv << mbo);
      dfs = (s32)cumul[s] - nv;
    }
    sym2[2 * s] = dnb;
    sym2[2 * s + 1] = (u32)dfs;
  }
}

// Bits << 8 to code a symbol of normalised count nv in a table of 2^tableLog cells: libzstd's
// FSE_bitCost (the number of state bits, interpolated linearly between the two powers of two
// around the count), integers only.  The entropy kernel computes the same for its own tables.
inline u32 bit_cost(int nv, u32 tableLog) {
  if (nv == 0) return ZH_DENT_IMPOSSIBLE;
  u32 const n = nv < 0 ? 1u : (u32)nv, T = 1u << tableLog;
  u32 const mbo = n == 1 ? tableLog : tableLog - highbit(n - 1);
  u32 const dnb = (mbo << 16) - (n << mbo);
  u32 const minNb = dnb >> 16, threshold = (minNb + 1) << 16;
  u32 const delta = threshold - (dnb + T);
  return ((minNb + 1) << ZH_DENT_COST_SHIFT) - ((delta << ZH_DENT_COST_SHIFT) >> tableLog);
}

// Huffman weights of a tree description (RFC 8878 §4.2.1) at p: direct 4-bit weights or an
// FSE-compressed run; returns the bytes used (0: malformed) and the weights but the last
inline size_t read_weights(const u8 *p, size_t avail, u8 *w, u32 *nw) {
  if (!avail) return 0;
  u32 const hb = p[0];
  if (hb >= 128) {
    u32 const n = hb - 127;
    size_t const bytes = (n + 1) / 2;
    if (1 + bytes > avail) return 0;
    for (u32 i = 0; i < n; i++) w[i] = (i & 1) ? (p[1 + i / 2] & 15) : (p[1 + i / 2] >> 4);
    *nw = n;
    return 1 + bytes;
  }
  if (hb == 0 || 1 + (size_t)hb > avail) return 0;
  const u8 *const c = p + 1;
  s16 norm[13];
  u32 maxSV = 0, L = 0;
  size_t const hs = read_ncount(c, hb, 12, 6, norm, &maxSV, &L);
  if (!hs || hs >= hb) return 0;
  // decoding table
  u32 const T = 1u << L, mask = T - 1, step = (T >> 1) + (T >> 3) + 3;
  u8 dsym[64], dnb[64];
  u16 dnew[64], next[13];
  u32 high = T - 1;
  for (u32 s = 0; s <= maxSV; s++) {
    if (norm[s] == -1) {
      dsym[high--] = (u8)s;
      next[s] = 1;
    } else {
      next[s] = (u16)norm[s];
    }
  }
  u32 pos = 0;
  for (u32 s = 0; s <= maxSV; s++)
    for (int i = 0; i < norm[s]; i++) {
      dsym[pos] = (u8)s;
      pos = (pos + step) & mask;
      while (pos > high) pos = (pos + step) & mask;
    }
  if (pos != 0) return 0;
  for (u32 u = 0; u < T; u++) {
    u32 const ns = next[dsym[u]]++;
    dnb[u] = (u8)(L - highbit(ns));
    dnew[u] = (u16)((ns << dnb[u]) - T);
  }
  // the bitstream, read backwards from its end mark
  const u8 *const bsrc = c + hs;
  size_t const bn = hb - hs;
  if (bsrc[bn - 1] == 0) return 0;
  long bits = (long)(8 * (bn - 1) + highbit(bsrc[bn - 1]));  // bits below the end mark
  auto read = [&](u32 n) -> u32 {  // the n bits below the cursor (zeros below the stream's start)
    u32 v = 0;
    for (u32 k = 0; k < n; k++) {
      bits--;
      u32 const b = bits >= 0 ? (bsrc[bits >> 3] >> (bits & 7)) & 1u : 0u;
      v = (v << 1) | b;
    }
    return v;
  };
  u32 s1 = read(L), s2 = read(L);
  if (bits < 0) return 0;
  u32 n = 0;
  for (;;) {
    if (n + 2 > 255) return 0;
    w[n++] = dsym[s1];
    s1 = dnew[s1] + read(dnb[s1]);
    if (bits < 0) { w[n++] = dsym[s2]; break; }
    w[n++] = dsym[s2];
    s2 = dnew[s2] + read(dnb[s2]);
    if (bits < 0) { w[n++] = dsym[s1]; break; }
  }
  *nw = n;
  return 1 + (size_t)hb;
}

// The whole entropy section of formatted dictionary d (n bytes, magic and ID in front) -> e.
// false: not a formatted dictionary, or malformed (zh::dict_layout refuses the same buffers,
// and a few more this parser needs decoded: Huffman weights that are no prefix code).
inline bool parse(const u8 *d, size_t n, ZhDictEnt *e, size_t *content_off) {
  memset(e, 0, sizeof(*e));
  if (n < 8) return false;
  u32 magic;
  memcpy(&magic, d, 4);
  if (magic != 0xEC30A437u) return false;
  size_t o = 8;
  // Huffman: weights -> code lengths -> codes (HUF_readCTable's canonical assignment)
  u8 w[256];
  u32 nw = 0;
  size_t const hs = read_weights(d + o, n - o, w, &nw);
  if (!hs || nw == 0 || nw > 255) return false;
  o += hs;
  u32 total = 0;
  for (u32 i = 0; i < nw; i++) {
    if (w[i] > 12) return false;
    total += w[i] ? 1u << (w[i] - 1) : 0u;
  }
  if (total == 0) return false;
  u32 const hlog = highbit(total) + 1;
  if (hlog > 12) return false;
  u32 const rest = (1u << hlog) - total;
  if (rest == 0 || (rest & (rest - 1))) return false;  // the last weight completes a power of two
  w[nw] = (u8)(highbit(rest) + 1);
  u32 const nsym = nw + 1;
  u32 perRank[14] = {0}, valRank[14] = {0};
  for (u32 s = 0; s < nsym; s++) {
    e->hnb[s] = w[s] ? (u8)(hlog + 1 - w[s]) : 0;
    perRank[e->hnb[s]]++;
  }
  if (perRank[hlog] < 2 || (perRank[hlog] & 1)) return false;  // (the longest codes come in pairs: HUF_readStats)
  {
    u32 mn = 0;
    for (u32 r = hlog; r > 0; r--) {
      valRank[r] = mn;
      mn += perRank[r];
      mn >>= 1;
    }
  }
  for (u32 s = 0; s < nsym; s++)
    if (e->hnb[s]) e->hval[s] = (u16)valRank[e->hnb[s]]++;
  e->huf_log = hlog;
  if (hlog <= 11)  // (the literal packer's fields hold codes of <= 11 bits, libzstd's own limit for literals)
    for (u32 s = 0; s < nsym; s++)
      if (e->hnb[s]) e->hmask[s >> 5] |= 1u << (s & 31);
  // OF, ML, LL tables in the dictionary's order; blob order LL, OF, ML
  static const u32 msv[3] = {31, 52, 35}, mlg[3] = {8, 9, 9}, slot[3] = {1, 2, 0};
  static const u32 st_off[3] = {0, 1024, 1536}, sy_off[3] = {2560, 2848, 3104}, nsy[3] = {36, 32, 53};
  for (int k = 0; k < 3; k++) {
    s16 norm[64];
    u32 maxSV = 0, L = 0;
    size_t const u = o < n ? read_ncount(d + o, n - o, msv[k], mlg[k], norm, &maxSV, &L) : 0;
    if (!u) return false;
    o += u;
    u32 const t = slot[k];
    int sum = 0;
    for (u32 s = 0; s <= maxSV; s++) sum += norm[s] < 0 ? 1 : norm[s];
    if (sum != (1 << L)) return false;
    u16 st[512];
    u32 sym2[2 * 64];
    build_ctable(st, sym2, nsy[t], norm, maxSV, L);
    memcpy(e->fse + st_off[t], st, sizeof(u16) << L);
    memcpy(e->fse + sy_off[t], sym2, 8 * nsy[t]);
    e->logs[t] = L;
    for (u32 s = 0; s < 64; s++) e->cost[t][s] = s <= maxSV ? bit_cost(norm[s], L) : ZH_DENT_IMPOSSIBLE;
  }
  if (o + 12 > n) return false;
  size_t const cn = n - o - 12;
  for (int k = 0; k < 3; k++) {
    u32 r;
    memcpy(&r, d + o + 4 * k, 4);
    if (r == 0 || r > cn) return false;
    e->reps[k] = r;
  }
  *content_off = o + 12;
  return true;
}
}  // namespace dent
}  // namespace zh

// zh_dict_finalize.h — raw content + entropy statistics -> a formatted RFC 8878 §5 dictionary
// (what libzstd calls ZDICT_finalizeDictionary).  The statistics are the four histograms the
// entropy kernel's statistics pass (ZH_F_STATS) collects over the samples; everything here is a
// few hundred integers on the host.  Header only and HIP free (zh_dict_entropy.h's companion).
#pragma once
#include <algorithm>
#include <queue>
#include <vector>

#include "zh_dict_entropy.h"

namespace zh {
namespace dfin {
using namespace zh::dent;

inline u64 rotl64(u64 v, int r) { return (v << r) | (v >> (64 - r)); }
// XXH64 (seed 0), for libzstd's Dictionary_ID rule
inline u64 xxh64(const u8 *p, size_t n) {
  u64 const P1 = 11400714785074694791ull, P2 = 14029467366897019727ull, P3 = 1609587929392839161ull, P4 = 9650029242287828579ull,
            P5 = 2870177450012600261ull;
  auto rd64 = [](const u8 *q) { u64 v; memcpy(&v, q, 8); return v; };
  auto rd32 = [](const u8 *q) { u32 v; memcpy(&v, q, 4); return v; };
  auto round = [&](u64 acc, u64 in) { return rotl64(acc + in * P2, 31) * P1; };
  const u8 *const end = p + n;
  u64 h;
  if (n >= 32) {
    u64 v1 = P1 + P2, v2 = P2, v3 = 0, v4 = 0 - P1;
    for (; p + 32 <= end; p += 32) {
      v1 = round(v1, rd64(p));
      v2 = round(v2, rd64(p + 8));
      v3 = round(v3, rd64(p + 16));
      v4 = round(v4, rd64(p + 24));
    }
    h = rotl64(v1, 1) + rotl64(v2, 7) + rotl64(v3, 12) + rotl64(v4, 18);
    for (u64 v : {v1, v2, v3, v4}) h = (h ^ round(0, v)) * P1 + P4;
  } else {
    h = P5;
  }
  h += (u64)n;
  for (; p + 8 <= end; p += 8) h = rotl64(h ^ round(0, rd64(p)), 27) * P1 + P4;
  if (p + 4 <= end) {
    h = rotl64(h ^ (rd32(p) * P1), 23) * P2 + P3;
    p += 4;
  }
  for (; p < end; p++) h = rotl64(h ^ (*p * P5), 11) * P1;
  h ^= h >> 33;
  h *= P2;
  h ^= h >> 29;
  h *= P3;
  h ^= h >> 32;
  return h;
}

// Huffman code lengths of counts (all > 0), at most maxBits: the plain Huffman tree, with the counts
// halved (rounding up) until it is shallow enough
inline void huf_lengths(const u32 *count, u32 n, u32 maxBits, u8 *len) {
  std::vector<u64> c(count, count + n);
  for (;;) {
    typedef std::pair<u64, u32> Node;  // (count, node): ties by node index, deterministic
    std::priority_queue<Node, std::vector<Node>, std::greater<Node>> q;
    std::vector<u32> parent(2 * n, 0);
    for (u32 s = 0; s < n; s++) q.push({c[s], s});
    u32 next = n;
    while (q.size() > 1) {
      Node const a = q.top();
      q.pop();
      Node const b = q.top();
      q.pop();
      parent[a.second] = parent[b.second] = next;
      q.push({a.first + b.first, next++});
    }
    u32 const root = next - 1;
    u32 deepest = 0;
    for (u32 s = 0; s < n; s++) {
      u32 dpt = 0;
      for (u32 x = s; x != root; x = parent[x]) dpt++;
      len[s] = (u8)dpt;
      deepest = std::max(deepest, dpt);
    }
    if (deepest <= maxBits) return;
    for (auto &v : c) v = (v + 1) >> 1;
  }
}

// counts -> normalised counts summing to 1 << log, every counted symbol at least 1
inline void normalize(const u32 *count, u32 n, u32 log, s16 *norm) {
  u64 total = 0;
  for (u32 s = 0; s < n; s++) total += count[s];
  int const T = 1 << log;
  int sum = 0;
  for (u32 s = 0; s < n; s++) {
    norm[s] = count[s] ? (s16)std::max<u64>(1, (u64)count[s] * (u64)T / total) : 0;
    sum += norm[s];
  }
  while (sum != T) {  // the remainder goes to (comes from) the most probable symbol, first one on ties
    u32 best = 0;
    for (u32 s = 1; s < n; s++)
      if (norm[s] > norm[best]) best = s;
    if (sum < T) {
      norm[best] = (s16)(norm[best] + (T - sum));
      sum = T;
    } else {
      norm[best]--;
      sum--;
    }
  }
}

// FSE_writeNCount (the entropy kernel's fse_write_ncount_wave, serially); returns the size, 0 on error
inline size_t write_ncount(u8 *out, size_t cap, const s16 *norm, u32 maxSV, u32 tableLog) {
  size_t o = 0;
  bool over = false;
  auto put2 = [&](u32 bs) {
    if (o + 2 > cap) { over = true; return; }
    out[o] = (u8)bs;
    out[o + 1] = (u8)(bs >> 8);
    o += 2;
  };
  int const tableSize = 1 << tableLog;
  int remaining = tableSize + 1, threshold = tableSize, nbBits = (int)tableLog + 1;
  u32 bitStream = tableLog - 5;
  int bitCount = 4;
  u32 symbol = 0;
  u32 const alphabetSize = maxSV + 1;
  bool previousIs0 = false;
  while (symbol < alphabetSize && remaining > 1) {
    if (previousIs0) {
      u32 start = symbol;
      while (symbol < alphabetSize && !norm[symbol]) symbol++;
      if (symbol == alphabetSize) break;
      while (symbol >= start + 24) {
        start += 24;
        bitStream += 0xFFFFu << bitCount;
        put2(bitStream);
        bitStream >>= 16;
      }
      while (symbol >= start + 3) {
        start += 3;
        bitStream += 3u << bitCount;
        bitCount += 2;
      }
      bitStream += (symbol - start) << bitCount;
      bitCount += 2;
      if (bitCount > 16) {
        put2(bitStream);
        bitStream >>= 16;
        bitCount -= 16;
      }
    }
    int count = norm[symbol++];
    int const max = (2 * threshold - 1) - remaining;
    remaining -= count < 0 ? -count : count;
    count++;
    if (count >= threshold) count += max;
    bitStream += (u32)count << bitCount;
    bitCount += nbBits;
    bitCount -= (count < max);
    previousIs0 = (count == 1);
    if (remaining < 1) return 0;
    while (remaining < threshold) {
      nbBits--;
      threshold >>= 1;
    }
    if (bitCount > 16) {
      put2(bitStream);
      bitStream >>= 16;
      bitCount -= 16;
    }
  }
  if (remaining != 1) return 0;
  put2(bitStream);
  if (over) return 0;
  return o - 2 + (size_t)(bitCount + 7) / 8;
}

// Huffman tree description of code lengths len[0..n) (n >= 2, the last symbol's weight implied):
// the weights FSE-compressed (HUF_writeCTable's first form).  Empty on failure.
inline std::vector<u8> huf_header(const u8 *len, u32 n) {
  u32 maxLen = 0;
  for (u32 s = 0; s < n; s++) maxLen = std::max<u32>(maxLen, len[s]);
  u32 const nw = n - 1;
  std::vector<u8> w(nw);
  u32 cnt[13] = {0};
  for (u32 s = 0; s < nw; s++) {
    w[s] = len[s] ? (u8)(maxLen + 1 - len[s]) : 0;
    if (w[s] > 12) return {};
    cnt[w[s]]++;
  }
  u32 mx = 12, distinct = 0;
  while (mx && !cnt[mx]) mx--;
  for (u32 v = 0; v <= mx; v++) distinct += cnt[v] != 0;
  if (distinct < 2) return {};
  u32 const L = 6;
  s16 norm[13];
  normalize(cnt, mx + 1, L, norm);
  std::vector<u8> out(1 + 512);
  size_t const hs = write_ncount(out.data() + 1, 64, norm, mx, L);
  if (!hs) return {};
  u16 st[64];
  u32 sym2[2 * 13];
  build_ctable(st, sym2, mx + 1, norm, mx, L);
  u64 acc = 0;
  u32 nbits = 0;
  size_t o = 1 + hs;
  auto add = [&](u32 v, u32 nb) {
    acc |= ((u64)v & ((1ull << nb) - 1ull)) << nbits;
    nbits += nb;
    while (nbits >= 8) {
      out[o++] = (u8)acc;
      acc >>= 8;
      nbits -= 8;
    }
  };
  auto init = [&](u32 sy) {
    u32 const dnb = sym2[2 * sy], dfs = sym2[2 * sy + 1];
    u32 const nbo = (dnb + (1u << 15)) >> 16;
    return (u32)st[(((nbo << 16) - dnb) >> nbo) + dfs];
  };
  auto step = [&](u32 &state, u32 sy) {
    u32 const dnb = sym2[2 * sy], dfs = sym2[2 * sy + 1];
    u32 const nb = (state + dnb) >> 16;
    add(state, nb);
    state = st[(state >> nb) + dfs];
  };
  int ip = (int)nw;
  u32 s1, s2;
  if (nw & 1) {
    s1 = init(w[--ip]);
    s2 = init(w[--ip]);
    step(s1, w[--ip]);
  } else {
    s2 = init(w[--ip]);
    s1 = init(w[--ip]);
  }
  while (ip > 0) {
    step(s2, w[--ip]);
    step(s1, w[--ip]);
  }
  add(s2, L);
  add(s1, L);
  add(1, 1);
  if (nbits) out[o++] = (u8)acc;
  size_t const body = o - 1;
  if (body >= 128) return {};
  out[0] = (u8)body;
  out.resize(o);
  return out;
}

constexpr u32 kStatsWords = 448;  // literal bytes [0, 256) | LL [256, 320) | OF [320, 384) | ML [384, 448) (zh_common.h ZH_STATS_*)

// The formatted dictionary of content (raw bytes) and the samples' statistics.  Every count
// starts at 1 as in ZDICT (libzstd refuses a dictionary in which an LL / ML code, or an offset
// code its content can reach, has no probability); Huffman depth <= 11; table logs 8 / 9 / 9 for
// OF / ML / LL; repcodes 1, 4, 8; dict_id 0: libzstd's rule over the content.  Empty on failure.
inline std::vector<u8> finalize(const u8 *content, size_t cn, const u32 *stats, u32 dict_id) {
  if (cn < 8) return {};
  u32 lit[256];
  for (u32 s = 0; s < 256; s++) lit[s] = stats[s] + 1;
  u8 len[256];
  huf_lengths(lit, 256, 11, len);
  std::vector<u8> hh = huf_header(len, 256);
  if (hh.empty()) {  // (all weights equal: no FSE description of one symbol) -- tilt one count
    lit[0] += 256;
    huf_lengths(lit, 256, 11, len);
    hh = huf_header(len, 256);
    if (hh.empty()) return {};
  }
  if (!dict_id) dict_id = (u32)(xxh64(content, cn) % ((1ull << 31) - 32768) + 32768);
  std::vector<u8> out(8);
  u32 const magic = 0xEC30A437u;
  memcpy(out.data(), &magic, 4);
  memcpy(out.data() + 4, &dict_id, 4);
  out.insert(out.end(), hh.begin(), hh.end());
  static const u32 base[3] = {320, 384, 256}, nsym[3] = {31, 53, 36}, logs[3] = {8, 9, 9};  // OF, ML, LL
  for (int k = 0; k < 3; k++) {
    u32 c[64];
    s16 norm[64];
    for (u32 s = 0; s < nsym[k]; s++) c[s] = stats[base[k] + s] + 1;
    normalize(c, nsym[k], logs[k], norm);
    u8 nc[256];
    size_t const u = write_ncount(nc, sizeof(nc), norm, nsym[k] - 1, logs[k]);
    if (!u) return {};
    out.insert(out.end(), nc, nc + u);
  }
  static const u32 reps[3] = {1, 4, 8};
  for (int k = 0; k < 3; k++) {
    u8 b[4];
    memcpy(b, &reps[k], 4);
    out.insert(out.end(), b, b + 4);
  }
  out.insert(out.end(), content, content + cn);
  return out;
}
}  // namespace dfin
}  // namespace zh

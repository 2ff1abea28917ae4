// dict_entropy_check.cpp — the host parser of a formatted dictionary's entropy section
// (csrc/zh_dict_entropy.h) on its own: a stand-alone program (its own main) for the sanitizers.
//
//   dict_entropy_check DICT CONTENT_OFFSET
//
// DICT is a formatted dictionary (the test passes libzstd's ZDICT_trainFromBuffer output),
// CONTENT_OFFSET where its content starts by an independent parser.  Checks the blob's invariants
// on the dictionary, then parses every truncated copy and every single-bit corruption of its
// entropy section from exactly-sized heap buffers: none may read out of bounds, and whatever
// still parses must keep the invariants.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "zh_dict_entropy.h"
#include "zh_dict_finalize.h"

using namespace zh::dent;

static int fail(const char *what, long a = 0, long b = 0) {
  std::printf("FAIL: %s (%ld, %ld)\n", what, a, b);
  return 1;
}

// invariants of a blob that parse() accepted for a dictionary of n bytes
static const char *check(const ZhDictEnt &e, size_t n, size_t off) {
  if (off < 8 + 1 + 3 + 12 || off > n) return "content offset";
  // Huffman: a complete prefix code (Kraft sum exactly 1), canonical values below 2^len, distinct
  u64 kraft = 0;
  u32 ncodes = 0;
  if (e.huf_log == 0 || e.huf_log > 12) return "huf_log";
  for (u32 s = 0; s < 256; s++) {
    u32 const l = e.hnb[s];
    bool const m = (e.hmask[s >> 5] >> (s & 31)) & 1;
    if (l > e.huf_log) return "code longer than huf_log";
    if (m && (!l || e.huf_log > 11)) return "mask without a code";
    if (e.huf_log <= 11 && !m && l) return "code without its mask bit";
    if (!l) continue;
    ncodes++;
    kraft += 1ull << (12 - l);
    if (e.hval[s] >> l) return "code value wider than its length";
    for (u32 t = 0; t < s; t++)
      if (e.hnb[t] == l && e.hval[t] == e.hval[s]) return "two symbols share a code";
  }
  if (ncodes < 2 || kraft != (1ull << 12)) return "not a complete prefix code";
  // FSE: states are a permutation of [T, 2T); costs impossible exactly where no state leads
  static const u32 st_off[3] = {0, 1024, 1536}, sy_off[3] = {2560, 2848, 3104}, nsy[3] = {36, 32, 53}, mlg[3] = {9, 8, 9};
  for (int t = 0; t < 3; t++) {
    u32 const L = e.logs[t], T = 1u << L;
    if (L < 5 || L > mlg[t]) return "table log";
    const u16 *st = (const u16 *)(e.fse + st_off[t]);
    std::vector<u8> seen(T, 0);
    for (u32 i = 0; i < T; i++) {
      if (st[i] < T || st[i] >= 2 * T || seen[st[i] - T]) return "states are no permutation";
      seen[st[i] - T] = 1;
    }
    const u32 *sy = (const u32 *)(e.fse + sy_off[t]);
    u32 possible = 0;
    for (u32 s = 0; s < 64; s++) {
      u32 const c = e.cost[t][s];
      if (c == ZH_DENT_IMPOSSIBLE) continue;
      if (s >= nsy[t]) return "cost for a symbol outside the alphabet";
      if (c == 0 || c > ((L + 1) << ZH_DENT_COST_SHIFT)) return "cost out of range";
      possible++;
      // the symbol's first state slot lies inside the table
      u32 const dnb = sy[2 * s];
      s32 const dfs = (s32)sy[2 * s + 1];
      u32 const nbo = (dnb + (1u << 15)) >> 16;
      u32 const idx = (((nbo << 16) - dnb) >> nbo) + (u32)dfs;
      if (idx >= T) return "initial state outside the table";
    }
    if (!possible) return "table without symbols";
  }
  for (int k = 0; k < 3; k++)
    if (e.reps[k] == 0 || e.reps[k] > n - off) return "repcode outside the content";
  return nullptr;
}

int main(int argc, char **argv) {
  if (argc < 3) return fail("usage: dict_entropy_check DICT CONTENT_OFFSET");
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return fail("cannot open the dictionary");
  std::vector<u8> d;
  for (int c; (c = std::fgetc(f)) != EOF;) d.push_back((u8)c);
  std::fclose(f);
  size_t const want_off = (size_t)std::strtoul(argv[2], nullptr, 10);

  ZhDictEnt e;
  size_t off = 0;
  if (!parse(d.data(), d.size(), &e, &off)) return fail("the dictionary does not parse");
  if (off != want_off) return fail("content offset", (long)off, (long)want_off);
  if (const char *w = check(e, d.size(), off)) return fail(w);
  u32 codes = 0;
  for (u32 s = 0; s < 256; s++) codes += e.hnb[s] != 0;
  std::printf("huffman: %u codes, longest %u; logs LL %u OF %u ML %u; reps %u %u %u; content at %zu\n", codes, e.huf_log, e.logs[0], e.logs[1],
              e.logs[2], e.reps[0], e.reps[1], e.reps[2], off);

  // truncated copies, each in a heap buffer of exactly its size
  size_t parsed = 0;
  for (size_t n = 0; n <= off + 16 && n <= d.size(); n++) {
    std::unique_ptr<u8[]> b(new u8[n ? n : 1]);
    if (n) memcpy(b.get(), d.data(), n);
    ZhDictEnt t;
    size_t o = 0;
    if (parse(b.get(), n, &t, &o)) {
      parsed++;
      if (n < off + 1) return fail("a dictionary cut inside its entropy section parsed", (long)n);
      if (const char *w = check(t, n, o)) return fail(w, (long)n);
    }
  }
  // every single-bit corruption of the entropy section (and of the magic)
  size_t ok = 0, bad = 0;
  {
    size_t const n = off + 64 <= d.size() ? off + 64 : d.size();
    std::unique_ptr<u8[]> b(new u8[n]);
    for (size_t i = 0; i < off; i++) {
      if (i >= 4 && i < 8) continue;  // (the Dictionary_ID: any value)
      for (int bit = 0; bit < 8; bit++) {
        memcpy(b.get(), d.data(), n);
        b[i] ^= (u8)(1 << bit);
        ZhDictEnt t;
        size_t o = 0;
        if (parse(b.get(), n, &t, &o)) {
          ok++;
          if (i < 4) return fail("a wrong magic parsed", (long)i);
          if (const char *w = check(t, n, o)) return fail(w, (long)i, bit);
        } else {
          bad++;
        }
      }
    }
  }
  std::printf("truncations parsed: %zu; corruptions accepted %zu, refused %zu\n", parsed, ok, bad);

  // finalisation (zh_dict_finalize.h): content + statistics -> a formatted dictionary that parses
  // back to the same code lengths, with every LL / ML / OF code given a probability
  u32 seed = 12345;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
  for (int shape = 0; shape < 4; shape++) {
    u32 stats[zh::dfin::kStatsWords] = {0};
    if (shape == 1) for (u32 i = 0; i < 8; i++) stats[(i * 37) & 255] += 1;            // one 8-byte sample
    if (shape == 2) for (u32 i = 0; i < zh::dfin::kStatsWords; i++) stats[i] = rnd() % 1000;
    if (shape == 3) for (u32 i = 0; i < zh::dfin::kStatsWords; i++) stats[i] = (rnd() % 7 == 0) ? rnd() % 5000000 : rnd() % 3;  // deep tree
    std::vector<u8> const content(d.begin() + (long)off, d.end());
    std::vector<u8> const fd = zh::dfin::finalize(content.data(), content.size(), stats, shape == 2 ? 77777u : 0u);
    if (fd.empty()) return fail("finalize failed", shape);
    ZhDictEnt t;
    size_t o = 0;
    if (!parse(fd.data(), fd.size(), &t, &o)) return fail("a finalised dictionary does not parse", shape);
    if (const char *w = check(t, fd.size(), o)) return fail(w, shape);
    if (fd.size() - o != content.size() || memcmp(fd.data() + o, content.data(), content.size())) return fail("content changed", shape);
    u32 id;
    memcpy(&id, fd.data() + 4, 4);
    if (shape == 2 ? id != 77777u : id < 32768u) return fail("dictionary id", shape, (long)id);
    if (t.huf_log > 11 || t.reps[0] != 1 || t.reps[1] != 4 || t.reps[2] != 8) return fail("huffman depth / repcodes", shape);
    for (u32 s2 = 0; s2 < 256; s2++)
      if (!t.hnb[s2]) return fail("a byte value without a code", shape, (long)s2);
    for (u32 s2 = 0; s2 < 36; s2++) if (t.cost[0][s2] == ZH_DENT_IMPOSSIBLE) return fail("LL code without probability", shape, (long)s2);
    for (u32 s2 = 0; s2 < 31; s2++) if (t.cost[1][s2] == ZH_DENT_IMPOSSIBLE) return fail("OF code without probability", shape, (long)s2);
    for (u32 s2 = 0; s2 < 53; s2++) if (t.cost[2][s2] == ZH_DENT_IMPOSSIBLE) return fail("ML code without probability", shape, (long)s2);
    if (t.logs[0] != 9 || t.logs[1] != 8 || t.logs[2] != 9) return fail("table logs", shape);
  }
  std::printf("finalised dictionaries parse back\n");
  std::printf("dict entropy parser OK\n");
  return 0;
}

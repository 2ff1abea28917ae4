// Stand-alone host check of the batched range read's arithmetic (csrc/zh_seek_ranges.h): the
// two-level search and the segment walk against a plain linear loop over the sizes, and the temp
// layout.  tests/test_seek_ranges_plan.py builds it with -fsanitize=address,undefined and runs
// it on the CPU.  Every array is exactly as long as the kernels' (ASan catches a read past it).
#include "zh_seek_ranges.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      printf("FAILED line %d: %s (table %s)\n", __LINE__, #c, g_name); \
      exit(1);                                                     \
    }                                                              \
  } while (0)

static const char *g_name = "";

struct Table {
  std::vector<uint64_t> d, start, ld, tbd;  // sizes; plain prefix sums; the scanned form
  uint64_t total = 0;
  explicit Table(std::vector<uint64_t> sizes) : d(std::move(sizes)) {
    for (uint64_t v : d) {
      start.push_back(total);
      total += v;
    }
    ld.resize(d.size());
    tbd.resize((d.size() + ZH_SEEK_TILE - 1) / ZH_SEEK_TILE);
    for (size_t i = 0; i < d.size(); i++) {
      if (i % ZH_SEEK_TILE == 0) tbd[i / ZH_SEEK_TILE] = start[i];
      ld[i] = start[i] - tbd[i / ZH_SEEK_TILE];
    }
  }
  ZhSeekIndex index() const { return ZhSeekIndex{ld.data(), tbd.data(), d.size(), total}; }
  uint64_t linear_cover(uint64_t pos) const {  // the entry with start <= pos < start + size
    for (size_t i = 0; i < d.size(); i++)
      if (start[i] <= pos && pos < start[i] + d[i]) return i;
    return ~0ull;
  }
};

static uint64_t g_searches = 0, g_walks = 0;

static void check_walk(const Table &t, uint64_t p0, uint64_t end) {
  ZhSeekIndex const x = t.index();
  // the plain loop: every entry with content, clipped to [p0, end)
  std::vector<ZhSeekSeg> want;
  for (size_t i = 0; i < t.d.size(); i++) {
    uint64_t const lo = std::max(t.start[i], p0), hi = std::min(t.start[i] + t.d[i], end);
    if (lo < hi) want.push_back(ZhSeekSeg{i, lo - t.start[i], lo, hi - lo});
  }
  uint64_t i = zh_seek_cover(x, p0), pos = p0;
  ZhSeekSeg s;
  size_t k = 0;
  while (zh_seek_next_seg(x, &i, &pos, end, &s)) {
    CHECK(k < want.size());
    CHECK(s.frame == want[k].frame && s.in_frame == want[k].in_frame && s.pos == want[k].pos && s.len == want[k].len);
    CHECK(s.len > 0 && s.in_frame + s.len <= t.d[s.frame]);
    k++;
  }
  CHECK(k == want.size() && pos == end);
  g_walks++;
}

static void check_table(const char *name, const Table &t) {
  g_name = name;
  ZhSeekIndex const x = t.index();
  CHECK(zh_seek_start(x, t.d.size()) == t.total);
  // every offset at a frame boundary and +-1 from it
  std::vector<uint64_t> edges;
  for (size_t i = 0; i <= t.d.size(); i++) {
    uint64_t const b = i < t.d.size() ? t.start[i] : t.total;
    CHECK(zh_seek_start(x, i) == b);
    for (int k = -1; k <= 1; k++)
      if ((k >= 0 || b > 0) && b + k < t.total) edges.push_back(b + k);
  }
  std::sort(edges.begin(), edges.end());
  edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
  bool const small = t.d.size() <= 64;
  for (uint64_t p : edges) {
    uint64_t const c = zh_seek_cover(x, p);
    g_searches++;
    CHECK(c < t.d.size() && t.d[c] > 0 && t.start[c] <= p && p < t.start[c] + t.d[c]);
    if (small) CHECK(c == t.linear_cover(p));
  }
  // ranges between edges: every pair for a small table, neighbours at several distances for a
  // large one, each cut into pieces as the scatter kernel cuts it
  auto range = [&](uint64_t a, uint64_t b) {  // content [a, b)
    CHECK(zh_seek_range_ok(a, b - a, t.total, b - a));
    for (uint64_t po = 0; po < b - a; po += ZH_SEEK_PIECE) check_walk(t, a + po, std::min(b, a + po + ZH_SEEK_PIECE));
  };
  size_t const steps[] = {1, 2, 3, 4, 7, 3000};
  for (size_t ia = 0; ia < edges.size(); ia++) {
    if (small) {
      for (size_t ib = ia; ib < edges.size(); ib++) range(edges[ia], edges[ib] + 1);
      continue;
    }
    // (the plain loop is linear in the table: all starts near a tile edge, every 7th elsewhere)
    uint64_t const in_tile = zh_seek_cover(x, edges[ia]) % ZH_SEEK_TILE;
    bool const near = in_tile < 6 || in_tile + 6 > ZH_SEEK_TILE || ia < 8 || ia + 8 > edges.size();
    if (!near && ia % 7) continue;
    for (size_t st : steps)
      if (ia + st < edges.size() && (st < 3000 || ia % 257 == 0)) range(edges[ia], edges[ia + st] + 1);
  }
  if (t.total) range(0, t.total);
  // pieces that begin or end exactly on a frame edge
  for (size_t i = 0; i < t.d.size() && (small || i % 97 == 0 || i + 3 > t.d.size()); i++)
    if (t.d[i]) {
      check_walk(t, t.start[i], t.start[i] + t.d[i]);
      if (t.start[i] + t.d[i] < t.total) check_walk(t, t.start[i], t.start[i] + t.d[i] + 1);
      if (t.start[i]) check_walk(t, t.start[i] - 1, t.start[i] + t.d[i]);
      check_walk(t, t.start[i], std::min(t.total, t.start[i] + ZH_SEEK_PIECE));
    }
  // verdicts at the content's end
  CHECK(zh_seek_range_ok(t.total, 0, t.total, 0));
  CHECK(!zh_seek_range_ok(t.total, 1, t.total, 8));
  CHECK(!zh_seek_range_ok(t.total + 1, 0, t.total, 8));
  CHECK(!zh_seek_range_ok(0, t.total + 1, t.total, ~0ull));
  CHECK(!zh_seek_range_ok(~0ull, 2, t.total, 8));  // offset + length wraps
  if (t.total >= 2) CHECK(!zh_seek_range_ok(0, 2, t.total, 1) && zh_seek_range_ok(t.total - 2, 2, t.total, 2));
}

static std::vector<uint64_t> sizes(size_t n, uint32_t seed, uint64_t lo, uint64_t hi, int zero_every) {
  std::vector<uint64_t> v(n);
  uint32_t s = seed;
  for (size_t i = 0; i < n; i++) {
    s = s * 1664525u + 1013904223u;
    v[i] = lo + (s >> 8) % (hi - lo + 1);
    if (zero_every && i % zero_every == (size_t)zero_every - 1) v[i] = 0;
  }
  return v;
}

static void check_layout() {
  g_name = "layout";
  size_t const fixed[] = {0, 1, 255, 256, 4097}, ns[] = {0, 1, 31, 32, 33, 1025, 2305}, rs[] = {1, 2, 63, 65, 65536}, js[] = {0, 1, 7, 2305},
               ds[] = {0, 1, 255, 256, 257, 4096, 65536}, decs[] = {0, 1, 1000};
  for (size_t f : fixed) for (size_t n : ns) for (size_t r : rs) for (size_t j : js) for (size_t d : ds) for (size_t dec : decs) {
    ZhSeekRangesLayout const L = zh_seek_ranges_layout(f, n, r, j, d, dec);
    size_t const beg[] = {0, L.bitmap, L.job_of_frame, L.first, L.last, L.staging, L.dec};
    size_t const len[] = {f, L.bitmap_bytes, n * 4, r * 4, r * 4, j * L.slot, dec};
    CHECK(L.bitmap_bytes * 8 >= n && L.slot >= d && L.slot >= 1 && L.slot % 256 == 0);
    for (int k = 0; k < 7; k++) {
      CHECK(beg[k] % 256 == 0);
      CHECK(beg[k] + len[k] + 255 <= L.total);  // inside the reported size wherever the 256-aligned base lands
      if (k) CHECK(beg[k - 1] + len[k - 1] <= beg[k]);  // in order, no overlap
    }
    // what sits in front of the staging slots does not depend on the jobs
    ZhSeekRangesLayout const P = zh_seek_ranges_layout(f, n, r, 0, 0, 0);
    CHECK(P.bitmap == L.bitmap && P.job_of_frame == L.job_of_frame && P.first == L.first && P.last == L.last && P.staging == L.staging);
    if (j) CHECK(zh_seek_ranges_layout(f, n, r, j - 1, d, dec).total + 256 <= L.total);  // one job fewer is at least a slot smaller
  }
}

int main() {
  // 1, 2, 1,023, 1,024, 1,025 and 2,305 entries: one tile, its edge, and three tiles
  for (size_t n : {1u, 2u, 1023u, 1024u, 1025u, 2305u}) {
    check_table("plain", Table(sizes(n, 7u + (uint32_t)n, 1, 700, 0)));
    check_table("equal 256", Table(std::vector<uint64_t>(n, 256)));
    check_table("one byte", Table(std::vector<uint64_t>(n, 1)));
    if (n > 2) check_table("zero every 3rd", Table(sizes(n, 11u + (uint32_t)n, 1, 40000, 3)));
  }
  // zero-size entries at the front, in the middle, doubled, and at the end
  check_table("zeros small", Table({0, 5, 0, 0, 7, 1, 0, 20000, 0}));
  check_table("zeros front doubled", Table({0, 0, 3, 9}));
  check_table("zeros end doubled", Table({3, 9, 0, 0}));
  check_table("single after zero", Table({0, 1}));
  check_table("single before zero", Table({1, 0}));
  {  // the same around the tile edge: entries 1,022..1,025 and a whole first tile of zeros
    auto v = sizes(2305, 99, 1, 300, 0);
    v[0] = 0; v[1022] = 0; v[1023] = 0; v[1024] = 0; v[1025] = 0; v[2047] = 0; v[2048] = 0; v[2304] = 0; v[2303] = 0;
    check_table("zeros at tile edges", Table(v));
    std::vector<uint64_t> w(2305, 0);
    for (size_t i = 1024; i < 2305; i += 5) w[i] = 100 + i % 50;
    check_table("first tile all zero", Table(w));
    std::vector<uint64_t> u(2305, 0);
    u[3] = 17; u[1023] = 5;
    check_table("last tiles all zero", Table(u));
  }
  check_table("large frames", Table(sizes(40, 5, 1, 70000, 7)));  // several pieces per frame
  check_layout();
  printf("seek ranges OK: %llu searches, %llu walks\n", (unsigned long long)g_searches, (unsigned long long)g_walks);
  return 0;
}

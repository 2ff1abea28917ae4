// dict_train_set_check.cpp — the grouped device trainer's formulation against the host trainer,
// without a GPU.  One call trains one dictionary per group of consecutive samples; this program
// runs such a call serially from the pieces of csrc/zh_dict_plan.h only: the group records
// (cover_groups), ids over the whole concatenation, the look-back clamped at the group's first
// position (cover_lookback), and the per-group state in the slots of cover_temp_layout, wave after
// wave, every live group of a wave taking one step in turn as the device's launches do.  Each
// group's bytes are compared with zh::cover_train on that group's samples alone, over the shapes
// of tests/test_gpu_dict_train_set.py.  It also checks that the slots of a wave do not overlap,
// that the layout lies inside its total, and that the reported temp size covers the layout of
// every d in [4, 8].  Stand-alone (own main); built with ASan + UBSan by
// tests/test_dict_train_set_plan.py.
#include "zh_dict.cpp"
#include "zh_dict_plan.h"

#include <cstdio>
#include <string>

namespace {
typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;

struct Rng {
  u64 s;
  u32 next() {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return (u32)(s >> 24);
  }
  u32 below(u32 n) { return n ? next() % n : 0; }
};

enum Kind { JSON, RANDOM, CONSTANT };

// records that share keys and a small vocabulary, so that d-mers repeat across samples
std::vector<u8> gen(Kind kind, size_t n, Rng &r) {
  std::vector<u8> o;
  if (kind == CONSTANT) return std::vector<u8>(n, 0x41);
  if (kind == RANDOM) {
    for (size_t i = 0; i < n; i++) o.push_back((u8)r.next());
    return o;
  }
  static const char *keys[] = {"\"id\":", "\"user_name\":", "\"timestamp\":", "\"status\":\"active\",", "\"tags\":[\"alpha\",\"beta\"],",
                               "\"payload\":{\"kind\":\"event\",\"value\":", "\"location\":\"eu-west\","};
  while (o.size() < n) {
    std::string s = "{";
    for (u32 f = 0, nf = 2 + r.below(5); f < nf; f++) {
      s += keys[r.below(7)];
      s += std::to_string(r.next() % 100000);
      s += ",";
    }
    s += "}\n";
    o.insert(o.end(), s.begin(), s.end());
  }
  o.resize(n);
  return o;
}

typedef std::vector<std::vector<u8>> Group;  // samples

Group many(Kind kind, size_t n, u32 lo, u32 hi, u64 seed) {
  Rng r{seed * 0x9E3779B97F4A7C15ull + 1}, sizes{seed + 77};
  Group v;
  for (size_t i = 0; i < n; i++) v.push_back(gen(kind, lo + sizes.below(hi - lo + 1), r));
  return v;
}

int failures = 0;

void fail(const char *name, const char *what) {
  printf("%-34s %s\n", name, what);
  failures++;
}

struct Range {
  size_t a, b;
};

// the layout's regions: inside [0, total - 256], in order, none overlapping another; the slots of
// each per-group array are `slots` disjoint strides that hold what a group needs
void check_layout(const char *name, const zh::CoverTempLayout &L, size_t N, size_t ns, size_t ng, size_t dict_size) {
  size_t const slots = ng < zh::kCoverGroupsInFlight ? ng : zh::kCoverGroupsInFlight;
  if (L.slots != slots) fail(name, "layout: slots");
  std::vector<Range> r;
  r.push_back({L.groups, L.groups + ng * sizeof(zh::CoverGroup)});
  r.push_back({L.ends, L.ends + ns * 4});
  r.push_back({L.dm, L.dm + N * 4});
  r.push_back({L.prev, L.prev + N * 2});
  for (size_t s = 0; s < slots; s++) r.push_back({L.ctl + s * sizeof(zh::CoverCtl), L.ctl + (s + 1) * sizeof(zh::CoverCtl)});
  for (size_t s = 0; s < slots; s++) r.push_back({L.freq + s * L.freq_stride, L.freq + s * L.freq_stride + ((size_t)4 << zh::kCoverHashBits)});
  for (size_t s = 0; s < slots; s++) r.push_back({L.diff + s * L.diff_stride, L.diff + s * L.diff_stride + L.ntiles * zh::kCoverScanTile * 8});
  for (size_t s = 0; s < slots; s++) r.push_back({L.tsum + s * L.tsum_stride, L.tsum + s * L.tsum_stride + L.ntiles * 8});
  for (size_t s = 0; s < slots; s++) r.push_back({L.tbest + s * L.tbest_stride, L.tbest + s * L.tbest_stride + L.ntiles * 16});
  for (size_t s = 0; s < slots; s++) r.push_back({L.dict + s * L.dict_stride, L.dict + s * L.dict_stride + dict_size});
  for (size_t i = 0; i < r.size(); i++) {
    if (r[i].a > r[i].b || r[i].b + 256 > L.total) fail(name, "layout: a region leaves the total");
    if (i && r[i].a < r[i - 1].b) fail(name, "layout: regions overlap");  // (they are listed in layout order)
  }
  for (size_t o : {L.groups, L.ends, L.dm, L.prev, L.ctl, L.freq, L.diff, L.tsum, L.tbest, L.dict})
    if (o & 255) fail(name, "layout: alignment");
}

// one grouped call, as the device runs it -> every group's bytes
std::vector<std::vector<u8>> plan_train_groups(const char *name, const std::vector<Group> &gs, size_t dict_size, u32 k, u32 d) {
  std::vector<u8> corpus;  // no padding: every read below stays inside it
  std::vector<size_t> sizes, counts, ends;
  for (auto const &g : gs) {
    counts.push_back(g.size());
    for (auto const &s : g) {
      corpus.insert(corpus.end(), s.begin(), s.end());
      sizes.push_back(s.size());
      ends.push_back(corpus.size());
    }
  }
  size_t const ng = gs.size(), ns = sizes.size(), N = corpus.size();
  std::vector<zh::CoverGroup> groups(ng);
  u64 const total = zh::cover_groups(sizes.data(), counts.data(), ng, dict_size, k, d, groups.data());
  if (total != N) fail(name, "cover_groups: total");
  size_t max_ntiles = 0;
  for (size_t g = 0; g < ng; g++) {
    zh::CoverGroup const &G = groups[g];
    size_t n = 0;
    for (auto const &s : gs[g]) n += s.size();
    if (G.plan.N != n || G.s1 - G.s0 != gs[g].size() || G.base != (G.s0 ? ends[G.s0 - 1] : 0) || G.slot != g % zh::kCoverGroupsInFlight ||
        G.ntiles != zh::cover_scan_tiles(G.plan) || (size_t)G.ntiles * zh::kCoverScanTile < G.plan.esz + 1)
      fail(name, "cover_groups: record");
    max_ntiles = std::max<size_t>(max_ntiles, G.ntiles);
  }
  zh::CoverTempLayout const L = zh::cover_temp_layout(N, ns, ng, max_ntiles, dict_size);
  check_layout(name, L, N, ns, ng, dict_size);
  // the reported size covers the layout of every d (the query does not know d)
  for (u32 dd = 4; dd <= 8; dd++) {
    std::vector<zh::CoverGroup> gd(ng);
    (void)zh::cover_groups(sizes.data(), counts.data(), ng, dict_size, k, dd, gd.data());
    size_t nt = 0;
    for (auto const &G : gd) nt = std::max<size_t>(nt, G.ntiles);
    if (zh::cover_temp_bytes(sizes.data(), ns, counts.data(), ng, dict_size, k) < zh::cover_temp_layout(N, ns, ng, nt, dict_size).total)
      fail(name, "cover_temp_bytes below the layout");
  }
  if (ng == 1 && zh::cover_temp_bytes(sizes.data(), ns, counts.data(), 1, dict_size, k) != zh::cover_temp_bytes(N, ns, dict_size, k))
    fail(name, "the single query differs from the grouped one");

  std::vector<std::vector<u8>> out(ng);
  std::vector<u8> arena(L.total);
  u32 *const dm = (u32 *)(arena.data() + L.dm);
  u16 *const prev = (u16 *)(arena.data() + L.prev);
  zh::CoverPlan const whole = zh::cover_plan(N, dict_size, k, d);
  // ids: one pass over the concatenation with the samples' ends
  for (size_t i = 0; i < whole.nd; i++) {
    size_t const si = (size_t)(std::upper_bound(ends.begin(), ends.end(), i) - ends.begin());
    dm[i] = zh::kCoverNone;
    if (i + whole.d > ends[si]) continue;
    u64 v = 0;
    for (u32 j = 0; j < whole.d; j++) v |= (u64)corpus[i + j] << (8 * j);
    dm[i] = zh::cover_hash(v, whole.mask);
  }
  // prevdist: one pass, the look-back stops at the first position of the group that holds i
  for (size_t i = 0; i < whole.nd; i++) {
    prev[i] = 0;
    if (dm[i] == zh::kCoverNone) continue;
    size_t lo = 0, hi = ng - 1;
    while (lo < hi) {
      size_t const mid = lo + ((hi - lo + 1) >> 1);
      if (groups[mid].base <= i) lo = mid;
      else hi = mid - 1;
    }
    u32 const maxj = zh::cover_lookback(whole.seg, i - groups[lo].base);
    for (u32 j = 1; j <= maxj; j++)
      if (dm[i - j] == dm[i]) {
        prev[i] = (u16)j;
        break;
      }
  }
  for (size_t w = 0; w < zh::cover_waves(ng); w++) {
    size_t const g0 = w * zh::kCoverGroupsInFlight, gn = std::min(zh::kCoverGroupsInFlight, ng - g0);
    // the wave's slots start clear
    memset(arena.data() + L.freq, 0, gn * L.freq_stride);
    memset(arena.data() + L.diff, 0, gn * L.diff_stride);
    for (size_t j = 0; j < gn; j++) {
      zh::CoverGroup const &G = groups[g0 + j];
      zh::CoverCtl *const ctl = (zh::CoverCtl *)(arena.data() + L.ctl) + G.slot;
      *ctl = zh::CoverCtl{(u32)dict_size, 0u, 0u, G.plan.empty ? 1u : 0u};
      if (G.plan.empty) continue;
      // freq = distinct (bucket, sample) pairs of the group, into the group's slot
      u32 *const freq = (u32 *)(arena.data() + L.freq + G.slot * L.freq_stride);
      std::vector<std::pair<u32, u32>> pairs;
      for (u32 s = G.s0; s < G.s1; s++) {
        size_t const a = s ? ends[s - 1] : 0, e = std::min<size_t>(ends[s], G.base + G.plan.nd);
        for (size_t i = a; i < e; i++)
          if (dm[i] != zh::kCoverNone) pairs.emplace_back(dm[i], s);
      }
      std::sort(pairs.begin(), pairs.end());
      pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
      for (auto const &q : pairs) freq[q.first]++;
    }
    // steps: every group that is not done takes one, from its own control words, until all are done
    for (bool all_done = false; !all_done;) {
      all_done = true;
      for (size_t j = 0; j < gn; j++) {
        zh::CoverGroup const &G = groups[g0 + j];
        zh::CoverPlan const &p = G.plan;
        zh::CoverCtl *const ctl = (zh::CoverCtl *)(arena.data() + L.ctl) + G.slot;
        if (ctl->done) continue;
        all_done = false;
        u32 *const freq = (u32 *)(arena.data() + L.freq + G.slot * L.freq_stride);
        u64 *const diff = (u64 *)(arena.data() + L.diff + G.slot * L.diff_stride);
        u8 *const dict = arena.data() + L.dict + G.slot * L.dict_stride;
        const u32 *const gdm = dm + G.base;
        const u16 *const gprev = prev + G.base;
        zh::CoverEpoch const ep = zh::cover_epoch(p, ctl->epoch);
        size_t const nw = ep.wmax - ep.b + 1;
        for (size_t i = ep.b; i < ep.end; i++) {
          if (gdm[i] == zh::kCoverNone || !freq[gdm[i]]) continue;
          size_t lo, hi;
          if (!zh::cover_range(i, gprev[i], p.seg, ep, lo, hi)) continue;
          diff[lo - ep.b] += freq[gdm[i]];
          diff[hi + 1 - ep.b] -= freq[gdm[i]];
        }
        u64 run = 0, best = 0;
        size_t bw = 0;
        for (size_t t = 0; t < (size_t)G.ntiles * zh::kCoverScanTile; t++) {  // the group's tiles, cleared for the next step
          run += diff[t];
          diff[t] = 0;
          if (t < nw && run > best) best = run, bw = t;
        }
        ctl->epoch = (u32)((ctl->epoch + 1) % p.epochs);
        if (best == 0) {
          if (++ctl->zero_run >= p.max_zero) ctl->done = 1;
          continue;
        }
        size_t sb = ep.b + bw, se = std::min(ep.end, sb + p.seg);
        while (sb < se && (gdm[sb] == zh::kCoverNone || freq[gdm[sb]] == 0)) sb++;
        while (se > sb && (gdm[se - 1] == zh::kCoverNone || freq[gdm[se - 1]] == 0)) se--;
        for (size_t i = sb; i < se; i++)
          if (gdm[i] != zh::kCoverNone) freq[gdm[i]] = 0;
        size_t const bytes = zh::cover_commit_bytes(sb, se, p.d, ctl->tail);
        if (bytes < p.d) {
          ctl->done = 1;
          continue;
        }
        ctl->tail -= (u32)bytes;
        ctl->zero_run = 0;
        memcpy(dict + ctl->tail, corpus.data() + G.base + sb, bytes);
        if (ctl->tail == 0) ctl->done = 1;
      }
    }
    for (size_t j = 0; j < gn; j++) {
      zh::CoverGroup const &G = groups[g0 + j];
      if (G.plan.empty) continue;
      const zh::CoverCtl *const ctl = (const zh::CoverCtl *)(arena.data() + L.ctl) + G.slot;
      const u8 *const dict = arena.data() + L.dict + G.slot * L.dict_stride;
      out[g0 + j].assign(dict + ctl->tail, dict + dict_size);
    }
  }
  return out;
}

// empty[g]: the group is meant to give nothing; every other group must give 256 .. dict_size bytes
void check(const char *name, const std::vector<Group> &gs, size_t dict_size, u32 k, u32 d, const std::vector<size_t> &empty = {}) {
  std::vector<std::vector<u8>> const plan = plan_train_groups(name, gs, dict_size, k, d);
  size_t differ = 0, small = 0, bytes = 0;
  for (size_t g = 0; g < gs.size(); g++) {
    std::vector<std::pair<const u8 *, size_t>> hs;
    for (auto const &s : gs[g]) hs.emplace_back(s.data(), s.size());
    std::vector<u8> const host = hs.empty() ? std::vector<u8>() : zh::cover_train(hs, dict_size, k, d);
    bool const want_empty = std::find(empty.begin(), empty.end(), g) != empty.end();
    if (host != plan[g]) differ++;
    if (want_empty ? host.size() >= 256 : (host.size() < 256 || host.size() > dict_size)) small++;
    bytes += host.size();
  }
  bool const ok = !differ && !small;
  printf("%-34s %4zu groups  %8zu bytes  %s\n", name, gs.size(), bytes,
         ok ? "equal" : differ ? "DIFFERENT" : "a group's size is not what the shape means");
  if (!ok) failures++;
}

Group marker_group(const std::vector<size_t> &at, size_t n, u64 seed) {
  Rng r{seed};
  std::vector<u8> a = gen(RANDOM, n, r);
  for (size_t p : at)
    for (u32 j = 0; j < 16; j++) a[p + j] = (u8)(0xA0 + j);
  return Group{a};
}
}  // namespace

int main() {
  // 1. mixed groups, one wave
  check("mixed, one wave",
        {many(JSON, 64, 300, 300, 1), many(JSON, 37, 100, 3000, 4), many(JSON, 1, 20000, 20000, 8), many(JSON, 300, 0, 40, 9),
         many(CONSTANT, 50, 2000, 2000, 7)},
        4096, 1024, 8);
  // 2. the group boundary: identical groups, and a marker across the boundary
  {
    Group const a = many(JSON, 30, 200, 2000, 21);
    check("A, A, A", {a, a, a}, 4096, 1024, 8);
    check("A, A, A k64 d6", {a, a, a}, 2048, 64, 6);
    for (u32 k : {64u, 1024u}) {
      size_t const seg = k - 8 + 1, n = 8192;
      for (size_t dist : {seg - 2, seg - 1, seg}) {
        // group 0 ends with the marker inside its last seg - 1 positions; group 1 has it `dist` after that
        size_t const p0 = n - 16 - 4;
        size_t const p1 = p0 + dist - n;  // local position in group 1
        std::string const nm = "marker k" + std::to_string(k) + " dist " + std::to_string(dist);
        check(nm.c_str(), {marker_group({100, p0}, n, 31), marker_group({p1, p1 + 3000}, n, 32)}, 4096, k, 8);
      }
    }
  }
  // 3. independent control state
  check("control state", {many(JSON, 40, 4096, 4096, 3), many(JSON, 3, 65536, 65536, 5), many(JSON, 1, 1000, 1000, 41), Group{}}, 65536, 1024, 8,
        {2, 3});
  // 4. more groups than slots
  {
    std::vector<Group> gs;
    for (u64 g = 0; g < 70; g++) gs.push_back(many(JSON, 20, 1024, 1024, 100 + (g == 64 ? 0 : g)));
    check("70 groups", gs, 2048, 1024, 8);
  }
  // 5. a long look-back
  check("2 x (20 x 6000) k40000", {many(JSON, 20, 6000, 6000, 14), many(JSON, 20, 6000, 6000, 15)}, 65536, 40000, 8);
  // 6. one group
  check("one group 200 x 1..5000", {many(JSON, 200, 1, 5000, 2)}, 16384, 1024, 8);
  // 7. zero-size samples at a group's edges and as a whole group
  {
    Group a = many(JSON, 20, 500, 500, 51), b = many(JSON, 20, 500, 500, 52);
    a.insert(a.begin(), std::vector<u8>());
    a.push_back(std::vector<u8>());
    b.insert(b.begin(), std::vector<u8>());
    b.push_back(std::vector<u8>());
    check("zero-size samples", {a, Group{{}, {}, {}}, b}, 4096, 1024, 8, {1});
  }
  // other d, and clamps
  check("d 4, k 2048", {many(JSON, 25, 1100, 1100, 12), many(JSON, 30, 1100, 1100, 13)}, 2048, 2048, 4);
  check("d clamp low, k clamp", {many(JSON, 20, 700, 700, 15), many(JSON, 20, 700, 700, 16)}, 1024, 3, 2);
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("dict train set plan OK\n");
  return 0;
}

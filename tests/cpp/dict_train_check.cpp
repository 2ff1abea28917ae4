// dict_train_check.cpp — the device trainer's formulation against the host trainer, without a GPU.
// Rebuilds the dictionary serially from the pieces of csrc/zh_dict_plan.h only (epoch geometry,
// the per-position [lo, hi] window ranges into a difference array, prefix sum, lowest-w arg-max,
// the commit rules) and compares it with zh::cover_train over the shape table of
// tests/test_gpu_dict_train.py.  Stand-alone (own main); built with ASan + UBSan by
// tests/test_dict_train_plan.py.
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

// zh::cover_train from the plan header's pieces: what the device kernels compute, run serially
std::vector<u8> plan_train(const std::vector<std::vector<u8>> &samples, size_t dict_size, u32 k, u32 d) {
  std::vector<u8> corpus;  // no padding: every read below stays inside it
  std::vector<size_t> ends;
  for (auto const &s : samples) {
    corpus.insert(corpus.end(), s.begin(), s.end());
    ends.push_back(corpus.size());
  }
  zh::CoverPlan const p = zh::cover_plan(corpus.size(), dict_size, k, d);
  if (p.empty) return {};
  // 1. ids
  std::vector<u32> dm(p.nd, zh::kCoverNone);
  for (size_t i = 0; i < p.nd; i++) {
    size_t const si = (size_t)(std::upper_bound(ends.begin(), ends.end(), i) - ends.begin());
    if (i + p.d > ends[si]) continue;
    u64 v = 0;
    for (u32 j = 0; j < p.d; j++) v |= (u64)corpus[i + j] << (8 * j);
    dm[i] = zh::cover_hash(v, p.mask);
  }
  // 2. freq = distinct (bucket, sample) pairs
  std::vector<u32> freq(1u << zh::kCoverHashBits, 0);
  {
    std::vector<std::pair<u32, u32>> pairs;
    for (size_t i = 0; i < p.nd; i++)
      if (dm[i] != zh::kCoverNone) pairs.emplace_back(dm[i], (u32)(std::upper_bound(ends.begin(), ends.end(), i) - ends.begin()));
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    for (auto const &q : pairs) freq[q.first]++;
  }
  // 3. prevdist
  std::vector<u16> prev(p.nd, 0);
  for (size_t i = 0; i < p.nd; i++) {
    if (dm[i] == zh::kCoverNone) continue;
    for (size_t j = 1; j < p.seg && j <= i; j++)
      if (dm[i - j] == dm[i]) {
        prev[i] = (u16)j;
        break;
      }
  }
  // 4 + 5. steps
  std::vector<u8> dict(dict_size);
  std::vector<u64> diff(p.esz + 2, 0);
  size_t tail = dict_size, e = 0;
  u32 zero_run = 0;
  for (;; e = (e + 1) % p.epochs) {
    zh::CoverEpoch const ep = zh::cover_epoch(p, e);
    size_t const nw = ep.wmax - ep.b + 1;
    std::fill(diff.begin(), diff.end(), 0);
    for (size_t i = ep.b; i < ep.end; i++) {
      if (dm[i] == zh::kCoverNone || !freq[dm[i]]) continue;
      size_t lo, hi;
      if (!zh::cover_range(i, prev[i], p.seg, ep, lo, hi)) continue;
      diff[lo - ep.b] += freq[dm[i]];
      diff[hi + 1 - ep.b] -= freq[dm[i]];
    }
    u64 run = 0, best = 0;
    size_t bw = 0;
    for (size_t w = 0; w < nw; w++) {
      run += diff[w];
      if (run > best) best = run, bw = w;
    }
    if (best == 0) {
      if (++zero_run >= p.max_zero) break;
      continue;
    }
    zero_run = 0;
    size_t sb = ep.b + bw, se = std::min(ep.end, sb + p.seg);
    while (sb < se && (dm[sb] == zh::kCoverNone || freq[dm[sb]] == 0)) sb++;
    while (se > sb && (dm[se - 1] == zh::kCoverNone || freq[dm[se - 1]] == 0)) se--;
    for (size_t i = sb; i < se; i++)
      if (dm[i] != zh::kCoverNone) freq[dm[i]] = 0;
    size_t const bytes = zh::cover_commit_bytes(sb, se, p.d, tail);
    if (bytes < p.d) break;
    tail -= bytes;
    memcpy(dict.data() + tail, corpus.data() + sb, bytes);
    if (tail == 0) break;
  }
  dict.erase(dict.begin(), dict.begin() + (ptrdiff_t)tail);
  return dict;
}

int failures = 0;

void check(const char *name, const std::vector<std::vector<u8>> &samples, size_t dict_size, u32 k, u32 d, long want_size = -1) {
  std::vector<std::pair<const u8 *, size_t>> hs;
  for (auto const &s : samples) hs.emplace_back(s.data(), s.size());
  std::vector<u8> const host = zh::cover_train(hs, dict_size, k, d), plan = plan_train(samples, dict_size, k, d);
  bool const ok = host == plan && (want_size < 0 || (size_t)want_size == host.size());
  printf("%-28s host %6zu  plan %6zu  %s\n", name, host.size(), plan.size(), ok ? "equal" : "DIFFERENT");
  if (!ok) failures++;
}

std::vector<std::vector<u8>> many(Kind kind, size_t n, u32 lo, u32 hi, u64 seed) {
  Rng r{seed * 0x9E3779B97F4A7C15ull + 1}, sizes{seed + 77};
  std::vector<std::vector<u8>> v;
  for (size_t i = 0; i < n; i++) v.push_back(gen(kind, lo + sizes.below(hi - lo + 1), r));
  return v;
}
}  // namespace

int main() {
  check("64 x 300", many(JSON, 64, 300, 300, 1), 4096, 1024, 8);
  check("200 x 1..5000", many(JSON, 200, 1, 5000, 2), 16384, 1024, 8);
  check("40 x 4096", many(JSON, 40, 4096, 4096, 3), 65536, 1024, 8);
  check("37 x 100..3000 k256 d6", many(JSON, 37, 100, 3000, 4), 8192, 256, 6);
  check("3 x 65536", many(JSON, 3, 65536, 65536, 5), 32768, 1024, 8);
  check("50 x 2000 random", many(RANDOM, 50, 2000, 2000, 6), 4096, 1024, 8);
  check("50 x 2000 constant", many(CONSTANT, 50, 2000, 2000, 7), 4096, 1024, 8, 1024);
  check("1 x 20000", many(JSON, 1, 20000, 20000, 8), 4096, 1024, 8);
  check("300 x 0..40", many(JSON, 300, 0, 40, 9), 4096, 1024, 8);
  check("512 x 4096", many(JSON, 512, 4096, 4096, 10), 16384, 1024, 8);
  check("30 x 500..9000 dict 128K", many(JSON, 30, 500, 9000, 11), 131072, 1024, 8);
  check("25 x 1100 k2048 d4", many(JSON, 25, 1100, 1100, 12), 2048, 2048, 4);
  check("1 x 1024 (N == k)", many(JSON, 1, 1024, 1024, 13), 256, 1024, 8, 256);
  check("1 x 1023 (N < k)", many(JSON, 1, 1023, 1023, 14), 256, 1024, 8, 0);
  check("d clamp low, k clamp", many(JSON, 20, 700, 700, 15), 1024, 3, 2);
  check("d clamp high", many(JSON, 20, 700, 700, 16), 1024, 64, 11);
  if (failures) {
    printf("%d shapes differ\n", failures);
    return 1;
  }
  printf("dict train plan OK\n");
  return 0;
}

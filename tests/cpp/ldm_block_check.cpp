// ldm_block_check.cpp — csrc/zh_ldm.h on the host, against vectors written by the numpy model
// (tests/golden/ldm_blocks.json, tests/golden/make_ldm_golden.py): the one-sequence block writer for
// every offset code 15..27 (and the limits), match lengths at every code boundary up to
// ZH_LDM_MIN_SEG, at ZH_LDM_MIN_SEG and at 32,768, both values of the last bit; the hash, sample
// predicate, slot and tag of every position of a 4 KiB buffer, its last 64 bytes included, rolled
// and from scratch; the table size rule.  Its own main; built with -fsanitize=address,undefined by
// tests/test_ldm_model.py.  usage: ldm_block_check <ldm_blocks.json>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "zh_ldm.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// value of "key": "..." in the flat JSON
static std::string field(const std::string &js, const char *key) {
  std::string const k = std::string("\"") + key + "\": \"";
  size_t const a = js.find(k);
  if (a == std::string::npos) { std::printf("missing %s\n", key); std::exit(2); }
  size_t const b = js.find('"', a + k.size());
  return js.substr(a + k.size(), b - a - k.size());
}
static std::vector<std::string> split(const std::string &s, char sep) {
  std::vector<std::string> out;
  std::stringstream ss(s);
  std::string t;
  while (std::getline(ss, t, sep)) out.push_back(t);
  return out;
}
static std::vector<uint8_t> unhex(const std::string &h) {
  std::vector<uint8_t> out(h.size() / 2);
  for (size_t i = 0; i < out.size(); i++) out[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
  return out;
}

int main(int argc, char **argv) {
  if (argc < 2) { std::printf("usage: %s ldm_blocks.json\n", argv[0]); return 2; }
  std::ifstream f(argv[1]);
  std::stringstream buf;
  buf << f.rdbuf();
  std::string const js = buf.str();

  // ---- blocks
  size_t nblocks = 0;
  bool seen_code[32] = {};
  for (auto const &line : split(field(js, "blocks"), ';')) {
    auto const t = split(line, ' ');
    uint32_t const ml = (uint32_t)std::stoul(t[0]), dist = (uint32_t)std::stoul(t[1]), last = (uint32_t)std::stoul(t[2]);
    std::vector<uint8_t> const want = unhex(t[3]);
    std::vector<uint8_t> got(ZH_LDM_BLOCK_MAX);  // exactly the documented bound: a longer write is an ASan error
    uint32_t const n = zh_ldm_write_block(got.data(), ml, dist, last);
    CHECK(n <= ZH_LDM_BLOCK_MAX && n == want.size() && std::memcmp(got.data(), want.data(), n) == 0, "block ml %u dist %u last %u: %u bytes, want %zu",
          ml, dist, last, n, want.size());
    uint32_t c = 0;
    while (((dist + 3u) >> (c + 1)) != 0) c++;
    seen_code[c] = true;
    nblocks++;
  }
  for (uint32_t c = 15; c <= 28; c++) CHECK(seen_code[c], "no vector for offset code %u", c);

  // ---- hash, predicate, slot, tag
  std::vector<uint8_t> const data = unhex(field(js, "buffer"));
  std::string const hs = field(js, "hashes"), sm = field(js, "samples"), sl = field(js, "slots"), tg = field(js, "tags");
  uint32_t const tlog = (uint32_t)std::stoul(field(js, "table_log"));
  size_t const npos = data.size() - ZH_LDM_HASH_BYTES + 1;
  CHECK(data.size() == 4096 && hs.size() == 16 * npos && sm.size() == npos && sl.size() == 4 * npos && tg.size() == 8 * npos, "vector sizes");
  uint64_t roll = 0;
  for (uint32_t i = 0; i + 1 < ZH_LDM_HASH_BYTES; i++) roll = zh_ldm_roll(roll, data[i]);
  size_t nsamples = 0;
  for (size_t p = 0; p < npos; p++) {
    roll = zh_ldm_roll(roll, data[p + ZH_LDM_HASH_BYTES - 1]);  // (the last position reads the buffer's last byte, none after it)
    uint64_t const want = std::stoull(hs.substr(16 * p, 16), nullptr, 16);
    uint64_t const scratch = zh_ldm_hash(data.data() + p);
    CHECK(roll == want && scratch == want, "hash at %zu: rolled %016llx scratch %016llx want %016llx", p, (unsigned long long)roll,
          (unsigned long long)scratch, (unsigned long long)want);
    CHECK(zh_ldm_is_sample(want) == (sm[p] == '1'), "sample predicate at %zu", p);
    CHECK(zh_ldm_slot(want, tlog) == std::stoul(sl.substr(4 * p, 4), nullptr, 16), "slot at %zu", p);
    CHECK(zh_ldm_tag(want) == std::stoul(tg.substr(8 * p, 8), nullptr, 16), "tag at %zu", p);
    nsamples += sm[p] == '1';
  }
  CHECK(nsamples > 0, "the buffer has no sample");

  // ---- table size
  for (auto const &line : split(field(js, "table_logs"), ';')) {
    auto const t = split(line, ' ');
    CHECK(zh_ldm_table_log(std::stoull(t[0]), (uint32_t)std::stoul(t[1])) == std::stoul(t[2]), "table log of %s / %s", t[0].c_str(), t[1].c_str());
  }
  CHECK(zh_ldm_max_dist(16) == 65536u && zh_ldm_max_dist(27) == (1u << 27) && zh_ldm_max_dist(29) == ZH_LDM_MAX_DIST && zh_ldm_max_dist(31) == ZH_LDM_MAX_DIST,
        "max distance");

  if (fails) { std::printf("%d failures\n", fails); return 1; }
  std::printf("ldm OK: %zu blocks, %zu positions, %zu samples\n", nblocks, npos, nsamples);
  return 0;
}

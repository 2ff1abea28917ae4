// Stand-alone host check of csrc/zh_litpack.h (K1's literal compaction): for all 16 literal masks
// and a set of byte patterns, the v_perm_b32 selector applied to the dword gives the masked bytes
// in order in the low bytes and zero above them.  Built with ASan + UBSan by
// tests/test_litpack.py; plain host code, no GPU.
#include <cstdint>
#include <cstdio>

#include "zh_litpack.h"

// every selector is a compile-time constant too
static_assert(zh_litpack_sel(0x0) == 0x07060504u && zh_litpack_sel(0xF) == 0x03020100u, "selector ends");
static_assert(zh_litpack_sel(0xA) == 0x05040301u && zh_litpack_sel(0x8) == 0x06050403u, "selector middles");
static_assert(zh_perm_b32_model(0x44332211u, 0xDDCCBBAAu, 0x0C0D0500u) == 0x00FF22AAu, "v_perm_b32 model");

int main() {
  const uint32_t patterns[] = {0x00000000u, 0xFFFFFFFFu, 0x04030201u, 0x80FF7F01u, 0xDEADBEEFu, 0x00FF00FFu, 0x01000000u, 0x61626364u};
  int bad = 0;
  for (uint32_t w : patterns)
    for (uint32_t m = 0; m < 16; m++) {
      uint32_t want = 0, k = 0;
      for (uint32_t i = 0; i < 4; i++)
        if ((m >> i) & 1u) want |= ((w >> (8 * i)) & 255u) << (8 * k++);
      uint32_t const sel = zh_litpack_sel(m), got = zh_litpack(w, m);
      bool ok = got == want;
      for (uint32_t j = 0; j < 4; j++) {  // selector bytes: the set bits' indices in order, then a zero byte's
        uint32_t const s = (sel >> (8 * j)) & 255u;
        ok = ok && (j < k ? s < 4 && ((m >> s) & 1u) : s >= 4 && s < 8);
      }
      if (!ok) {
        std::printf("mask %x dword %08x: selector %08x gives %08x, want %08x\n", m, w, sel, got, want);
        bad++;
      }
    }
  if (bad) return 1;
  std::printf("litpack OK\n");
  return 0;
}

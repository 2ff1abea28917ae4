// Stand-alone host check of the seek-table header (csrc/zh_seek_format.h): encode, parse and
// validate over exactly sized buffers.  tests/test_seekable_format.py builds it with
// -fsanitize=address,undefined and runs it on the CPU.
#include "zh_seek_format.h"
#include <cassert>
#include <cstdio>
#include <cstring>
#include <vector>
int main() {
  for (int ck = 0; ck < 2; ck++)
    for (uint64_t n : {0ull, 1ull, 7ull, 1025ull}) {
      uint64_t tb = zh_seek_table_bytes(n, ck);
      std::vector<uint8_t> t(tb);  // exact size: ASan catches any byte outside
      zh_seek_write_header(t.data(), n, ck);
      for (uint64_t i = 0; i < n; i++) zh_seek_write_entry(t.data() + 8 + i * zh_seek_entry_bytes(ck), (uint32_t)(i + 1), (uint32_t)(i * 3), ck, (uint32_t)(i * 77));
      zh_seek_write_footer(t.data() + tb - 9, n, ck);
      ZhSeekFooter f;
      assert(zh_seek_parse_footer(t.data() + tb - 9, tb, &f) == 0);
      assert(f.n == n && f.table == tb && (int)f.checksums == ck);
      assert(zh_seek_check_header(t.data(), &f) == 0);
      // damaged: magic, reserved bits, N beyond the buffer, N beyond the limit
      auto u = t; u[tb - 1] ^= 1; assert(zh_seek_parse_footer(u.data() + tb - 9, tb, &f) == 6);
      u = t; u[tb - 5] |= 0x40; assert(zh_seek_parse_footer(u.data() + tb - 9, tb, &f) == 6);
      u = t; zh_seek_st32(u.data() + tb - 9, (uint32_t)n + 1); assert(zh_seek_parse_footer(u.data() + tb - 9, tb, &f) == 6);
      u = t; zh_seek_st32(u.data() + tb - 9, 0xFFFFFFFFu); assert(zh_seek_parse_footer(u.data() + tb - 9, tb, &f) == 6);
      u = t; zh_seek_st32(u.data() + 4, 1); assert(zh_seek_parse_footer(u.data() + tb - 9, tb, &f) == 0 && zh_seek_check_header(u.data(), &f) == 6);
    }
  ZhSeekFooter f; uint8_t small[16] = {0};
  assert(zh_seek_parse_footer(small + 7, 16, &f) == 6);
  puts("seek format OK");
}

// Host check of the block-descriptor rule (csrc/zh_block_plan.h): walks frame sizes x levels x
// dictionaries x history x padding and asserts the properties every consumer of the descriptors
// relies on, without restating the rule.  A stand-alone program (its own main) built with
// ASan + UBSan by tests/test_block_plan.py; prints "block plan OK".
#include "zh_block_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int fails = 0;
#define CHECK(c)                                                                                               \
  do {                                                                                                         \
    if (!(c)) {                                                                                                \
      if (fails++ < 20) printf("FAIL %s:%d %s  [size %llu level %d dict %u hist %u extra %u]\n", __FILE__, __LINE__, #c, \
                               (unsigned long long)g_size, g_level, g_dict, g_hist, g_extra);                  \
    }                                                                                                          \
  } while (0)
static u64 g_size;
static int g_level;
static u32 g_dict, g_hist, g_extra;

int main() {
  const u64 sizes[] = {1, 2, 32767, 32768, 32769, 65535, 65536, 65537, 98304, 98305, 163840, 1u << 20};
  const int levels[] = {1, 4, 5, 22};
  const u32 dicts[] = {0, 1024, 40 * 1024, 200 * 1024};
  const u64 caps[] = {1000, 5ull << 30};
  const u32 first_slot = 7, index = 3, dict_id = 0xABCD1234u;
  std::vector<u8> src((1u << 20) + 8 * 65536), dict(200 * 1024), out(16), staging((size_t)(first_slot + 48) * ZH_STAGE_SLOT);
  long walked = 0;
  for (u64 size : sizes)
    for (int level : levels)
      for (u32 dict_n : dicts)
        for (u32 hist = 0; hist < 2; hist++)
          for (u32 extra = 0; extra < 4; extra += 3)  // bpi = the frame's block count, and 3 more
            for (u64 cap : caps) {
              g_size = size, g_level = level, g_dict = dict_n, g_hist = hist, g_extra = extra;
              ZhBatchPlan p{};
              p.flags = ZH_F_CHECKSUM;
              p.hist = hist;
              if (dict_n) p.dict = dict.data(), p.dict_n = dict_n, p.dict_id = dict_id;
              p.staging = staging.data();
              p.out_cap = cap;
              ZhPlanItem const it{src.data(), size, index, level, out.data()};
              bool invalid = true;
              ZhItemDesc const id = zh_item_desc(p, it, first_slot, &invalid);
              CHECK(!invalid && id.dst == out.data() && id.cap == cap && id.first_block == first_slot && id.nblocks >= 1);
              bool const deep = level >= ZH_DEEP_LEVEL;
              u32 const bpi = id.nblocks + extra;
              CHECK(bpi <= 48);
              u64 covered = 0;
              u32 active = 0, firsts = 0, lasts = 0;
              for (u32 k = 0; k < bpi; k++) {
                ZhBlockDesc const d = zh_block_desc(p, it, k, first_slot + k);
                walked++;
                CHECK(d.frame_size == size && d.item == index);
                CHECK((d.flags & ZH_F_CHECKSUM) && !(d.flags & (ZH_F_LDM | ZH_F_DICTENT | ZH_F_STATS)));
                CHECK(!!(d.flags & ZH_F_DEEP) == deep);
                CHECK(!!(d.flags & ZH_F_DICT) == (dict_n != 0) && d.dict_id == (dict_n ? dict_id : 0u));
                if (d.n == 0) {  // a padding slot: only behind the frame's blocks
                  CHECK(covered == size && k >= id.nblocks);
                  continue;
                }
                CHECK(k == active && k < id.nblocks);  // the active blocks are the first slots
                active++;
                CHECK(d.src == src.data() + covered && d.n <= (u32)ZH_BLOCK_MAX);  // they tile the frame
                covered += d.n;
                firsts += !!(d.flags & ZH_F_FIRST);
                lasts += !!(d.flags & ZH_F_LAST);
                CHECK(!!(d.flags & ZH_F_FIRST) == (k == 0));
                CHECK(!!(d.flags & ZH_F_LAST) == (covered == size));
                CHECK(!!(d.flags & ZH_F_DIRECT) == (id.nblocks == 1));
                if (id.nblocks == 1) {
                  CHECK(d.dst == out.data() && d.dst_cap == (cap > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)cap));
                } else {
                  CHECK(d.dst == staging.data() + (size_t)(first_slot + k) * ZH_STAGE_SLOT && d.dst_cap == ZH_STAGE_SLOT);
                }
                if (k == 0) {
                  if (dict_n) {  // the content's tail, as much of it as the matcher can stage
                    CHECK(d.pre + d.pre_n == dict.data() + dict_n && d.pre >= dict.data());
                    if (deep) CHECK(d.pre_n <= (u32)ZH_DEEP_PRE && (d.pre_n == dict_n || d.pre_n == (u32)ZH_DEEP_PRE));
                    else CHECK(d.pre_n + d.n <= (u32)ZH_BLOCK_MAX && (d.pre_n == dict_n || d.pre_n + d.n == (u32)ZH_BLOCK_MAX));
                  } else {
                    CHECK(d.pre == nullptr && d.pre_n == 0);
                  }
                } else if (hist) {  // the 32 KiB of the frame in front of the block
                  CHECK(d.pre == d.src - ZH_HIST_BLOCK && d.pre_n == (u32)ZH_HIST_BLOCK && d.pre >= src.data());
                  CHECK(d.pre_n + d.n <= (u32)ZH_BLOCK_MAX);
                } else {
                  CHECK(d.pre == nullptr && d.pre_n == 0);
                }
              }
              CHECK(covered == size && active == id.nblocks && firsts == 1 && lasts == 1);
              // one block up to 64 KiB, except that a dictionary frame over 32 KiB splits below ZH_DEEP_LEVEL
              if (size <= (u64)ZH_HIST_BLOCK) CHECK(id.nblocks == 1);
              else if (size <= (u64)ZH_BLOCK_MAX) CHECK((id.nblocks > 1) == (dict_n != 0 && !deep));
              else CHECK(id.nblocks > 1);
            }
  {  // an empty item: invalid, no blocks, every slot inactive
    g_size = 0;
    ZhBatchPlan p{};
    p.staging = staging.data();
    ZhPlanItem const it{src.data(), 0, index, 3, out.data()};
    bool invalid = false;
    ZhItemDesc const id = zh_item_desc(p, it, first_slot, &invalid);
    CHECK(invalid && id.nblocks == 0);
    CHECK(zh_block_desc(p, it, 0, first_slot).n == 0 && zh_block_desc(p, it, 1, first_slot + 1).n == 0);
  }
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("block plan OK (%ld descriptors)\n", walked);
  return 0;
}

// Host check of the per-item prefix in the block-descriptor rule (csrc/zh_block_plan.h) and of the
// stream window arithmetic (csrc/zh_stream_window.h).  A stand-alone program (its own main) built
// with ASan + UBSan by tests/test_prefix_plan.py; prints "prefix plan OK".
//
// Descriptor rule: for sizes x levels x prefix lengths x padding slots, an item with a prefix has,
// slot for slot, the descriptors the rule gives an item without one in a batch whose
// ZhBatchPlan::dict is that prefix with dict_id 0; an item without a prefix has the descriptors of a
// dictionary-less batch, padded with inactive slots.
// Window function: zh_window_move and zh_copy_split drive a copy over real buffers (bytes at the
// ends, 16-byte pieces in the middle, as zh_window_update_kernel moves them), compared with a byte
// loop, for every alignment of source and destination.
#include "zh_block_plan.h"
#include "zh_stream_window.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static int fails = 0;
static char g_where[160];
#define CHECK(c)                                                                         \
  do {                                                                                   \
    if (!(c)) {                                                                          \
      if (fails++ < 20) printf("FAIL %s:%d %s  [%s]\n", __FILE__, __LINE__, #c, g_where); \
    }                                                                                    \
  } while (0)

static bool same_desc(const ZhBlockDesc &a, const ZhBlockDesc &b) {
  return a.src == b.src && a.dst == b.dst && a.frame_size == b.frame_size && a.n == b.n && a.item == b.item && a.dst_cap == b.dst_cap &&
         a.flags == b.flags && a.pre == b.pre && a.pre_n == b.pre_n && a.dict_id == b.dict_id;
}
static bool same_item(const ZhItemDesc &a, const ZhItemDesc &b) {
  return a.dst == b.dst && a.cap == b.cap && a.first_block == b.first_block && a.nblocks == b.nblocks;
}

static long check_rule() {
  const u64 sizes[] = {1, 32767, 32768, 32769, 65536, 65537, 163840};
  const int levels[] = {1, 3, 4, 5, 9};
  const u64 prefixes[] = {0, 1, 32767, 32768, 65535, 65536, 200000};
  const u32 first_slot = 5, index = 2;
  std::vector<u8> src(163840 + 65536), pre(200000), out(16), staging((size_t)(first_slot + 16) * ZH_STAGE_SLOT);
  long walked = 0;
  for (u64 size : sizes)
    for (int level : levels)
      for (u64 pn : prefixes)
        for (u32 hist = 0; hist < 2; hist++)
          for (u32 extra = 0; extra < 4; extra += 3) {
            snprintf(g_where, sizeof g_where, "size %llu level %d prefix %llu hist %u extra %u", (unsigned long long)size, level,
                     (unsigned long long)pn, hist, extra);
            ZhBatchPlan p{};  // the prefix batch: no batch dictionary
            p.flags = ZH_F_CHECKSUM;
            p.hist = hist;
            p.staging = staging.data();
            p.out_cap = 1u << 20;
            ZhBatchPlan q = p;  // the batch the unchanged rule is asked about: the prefix as its dictionary, dict_id 0
            if (pn) q.dict = pre.data(), q.dict_n = (u32)pn, q.dict_id = 0;
            ZhPlanItem const plain{src.data(), size, index, level, out.data()};
            ZhPlanItem with = plain;
            with.pre = pn ? pre.data() : nullptr;
            with.pre_n = pn;
            bool inv_a = true, inv_b = true;
            ZhItemDesc const ia = zh_item_desc(p, with, first_slot, &inv_a), ib = zh_item_desc(q, plain, first_slot, &inv_b);
            CHECK(!inv_a && !inv_b && same_item(ia, ib));
            // the batch's blocks per item: those of the largest chunk with the split applied, and more
            u32 const bpi = (u32)zh_frame_blocks(size, zh_split_dict(level, true)) + extra;
            CHECK(ia.nblocks <= bpi && bpi <= 16);
            u32 active = 0;
            for (u32 k = 0; k < bpi; k++) {
              ZhBlockDesc const a = zh_block_desc(p, with, k, first_slot + k), b = zh_block_desc(q, plain, k, first_slot + k);
              walked++;
              CHECK(same_desc(a, b));
              CHECK(!!(a.flags & ZH_F_DICT) == (pn != 0) && a.dict_id == 0);
              CHECK((a.n == 0) == (k >= ia.nblocks));  // padding behind the frame's blocks
              active += a.n != 0;
              if (k == 0 && pn) {  // the tail that fits
                u32 const room = level >= ZH_DEEP_LEVEL ? (u32)ZH_DEEP_PRE : (u32)ZH_BLOCK_MAX - a.n;
                CHECK(a.pre + a.pre_n == pre.data() + pn && a.pre_n == (pn < room ? (u32)pn : room));
              }
              if (pn == 0 && k == 0) CHECK(a.pre == nullptr && a.pre_n == 0 && !(a.flags & ZH_F_DICT));
            }
            CHECK(active == ia.nblocks);
            // without a prefix: one block up to 64 KiB; with one below ZH_DEEP_LEVEL: 32 KiB blocks over 32 KiB
            if (size <= (u64)ZH_BLOCK_MAX) CHECK((ia.nblocks > 1) == (pn != 0 && level < ZH_DEEP_LEVEL && size > (u64)ZH_HIST_BLOCK));
          }
  {  // a prefix length without a pointer: invalid, every slot inactive; its neighbours' rule is untouched
    snprintf(g_where, sizeof g_where, "null prefix");
    ZhBatchPlan p{};
    p.staging = staging.data();
    ZhPlanItem bad{src.data(), 40000, index, 3, out.data()};
    bad.pre_n = 100;
    bool invalid = false;
    (void)zh_item_desc(p, bad, first_slot, &invalid);
    CHECK(invalid);
    for (u32 k = 0; k < 3; k++) CHECK(zh_block_desc(p, bad, k, first_slot + k).n == 0);
    ZhPlanItem empty{src.data(), 0, index, 3, out.data()};
    empty.pre = pre.data(), empty.pre_n = 100;
    invalid = false;
    (void)zh_item_desc(p, empty, first_slot, &invalid);
    CHECK(invalid && zh_block_desc(p, empty, 0, first_slot).n == 0);
  }
  return walked;
}

// window ++ chunk moved as the kernel moves it: head bytes, 16-byte pieces at aligned destinations, tail bytes
static void split_copy(u8 *dst, const u8 *src, u64 n) {
  ZhCopySplit const s = zh_copy_split((uintptr_t)dst, n);
  CHECK(s.head + 16 * s.vec + s.tail == n && s.head < 16 && s.tail < 16);
  for (u64 i = 0; i < s.head; i++) dst[i] = src[i];
  for (u64 v = 0; v < s.vec; v++) {
    CHECK(((uintptr_t)(dst + s.head + 16 * v) & 15u) == 0);
    memcpy(dst + s.head + 16 * v, src + s.head + 16 * v, 16);
  }
  for (u64 i = s.head + 16 * s.vec; i < n; i++) dst[i] = src[i];
}

static long check_window() {
  const u64 W = ZH_STREAM_WINDOW;
  const u64 lens[] = {0, 1, 65535, 65536}, ns[] = {0, 1, 65535, 65536, 65537, 200000};
  long walked = 0;
  // exact-size heap buffers (ASan sees any byte outside them), bases aligned to 16
  for (u64 len : lens)
    for (u64 n : ns)
      for (u32 sa = 0; sa < 16; sa++)
        for (u32 da = 0; da < 16; da++) {
          snprintf(g_where, sizeof g_where, "len %llu n %llu src align %u dst align %u", (unsigned long long)len, (unsigned long long)n, sa, da);
          u8 *const old_base = (u8 *)aligned_alloc(16, (size_t)((len + sa + 15) / 16 * 16 + 16));
          u8 *const chunk_base = (u8 *)aligned_alloc(16, (size_t)((n + sa + 15) / 16 * 16 + 16));
          u8 *const next_base = (u8 *)aligned_alloc(16, (size_t)((W + da + 15) / 16 * 16 + 16));
          u8 *const old = old_base + sa, *const chunk = chunk_base + sa, *const next = next_base + da;
          for (u64 i = 0; i < len; i++) old[i] = (u8)(i * 7 + 1);
          for (u64 i = 0; i < n; i++) chunk[i] = (u8)(i * 13 + 5);
          // the byte loop: the last <= W bytes of old ++ chunk
          u64 const total = len + n, want_n = total < W ? total : W;
          std::vector<u8> want((size_t)want_n);
          for (u64 i = 0; i < want_n; i++) {
            u64 const g = total - want_n + i;
            want[(size_t)i] = g < len ? old[g] : chunk[g - len];
          }
          ZhWindowMove const m = zh_window_move(len, n, W);
          CHECK(m.keep + m.take == want_n && m.keep_from + m.keep == len && m.take_from + m.take == n);
          split_copy(next, old + m.keep_from, m.keep);
          split_copy(next + m.keep, chunk + m.take_from, m.take);
          CHECK(want_n == 0 || memcmp(next, want.data(), (size_t)want_n) == 0);
          free(old_base), free(chunk_base), free(next_base);
          walked++;
        }
  return walked;
}

int main() {
  long const a = check_rule(), b = check_window();
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("prefix plan OK (%ld descriptors, %ld window moves)\n", a, b);
  return 0;
}

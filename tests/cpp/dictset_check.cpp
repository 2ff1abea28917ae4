// Host check of the dictionary set's HIP-free parts (csrc/zh_dictset.h) and of its place in the
// block-descriptor rule (csrc/zh_block_plan.h).  A stand-alone program (its own main) built with
// ASan + UBSan by tests/test_dictset_plan.py; prints "dictset OK".
//
// Lookup: zh_dictset_find against a linear scan over sorted ID arrays of 0, 1, 2, 3, 4,095 and 4,096
// IDs -- every ID present, the first and last, every gap between neighbours, below the first, above
// the last, and IDs 0, 1 and 0xFFFFFFFF.
// Creation: zh_dictset_sort_ids sorts the non-zero IDs with their indices, refuses two entries with
// the same non-zero ID and a count outside 1 .. ZH_DICTSET_MAX, and accepts several ID-0 entries.
// Descriptor rule: an item planned against entry e (zh_dictset_plan_item) has, slot for slot, the
// descriptors the rule gives an item in a batch whose ZhBatchPlan::dict is that entry's content
// with its dict_id; index -1 the dictionary-less descriptors plus padding; a bad index only
// inactive slots and an invalid item.
#include "zh_dictset.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

static int fails = 0;
static char g_where[200];
#define CHECK(c)                                                                         \
  do {                                                                                   \
    if (!(c)) {                                                                          \
      if (fails++ < 20) printf("FAIL %s:%d %s  [%s]\n", __FILE__, __LINE__, #c, g_where); \
    }                                                                                    \
  } while (0)

static int32_t linear_find(const std::vector<ZhDictSetId> &ids, u32 id) {
  if (id == 0) return -1;
  for (const ZhDictSetId &e : ids)
    if (e.id == id) return (int32_t)e.index;
  return -1;
}

static long check_find() {
  long probes = 0;
  const size_t counts[] = {0, 1, 2, 3, 4095, 4096};
  for (int variant = 0; variant < 3; variant++)
    for (size_t n : counts) {
      // exact-size heap array: ASan sees a read past either end
      std::vector<ZhDictSetId> ids(n);
      for (size_t i = 0; i < n; i++) {
        // variant 0: spread IDs with gaps; 1: starts at 1, dense then sparse; 2: ends at 0xFFFFFFFF
        u32 id = variant == 0 ? (u32)(1000u + 977u * i + (i * i) % 7u)
                 : variant == 1 ? (u32)(1u + (i < 8 ? i : 8 + 3 * (i - 8)))
                                : (u32)(0xFFFFFFFFu - 5u * (u32)(n - 1 - i));
        ids[i] = ZhDictSetId{id, (u32)((i * 2654435761u) % (n ? n : 1))};  // indices in no order
      }
      for (size_t i = 1; i < n; i++) CHECK(ids[i - 1].id < ids[i].id);
      snprintf(g_where, sizeof g_where, "find variant %d n %zu", variant, n);
      auto probe = [&](u32 id) {
        probes++;
        CHECK(zh_dictset_find(ids.data(), (u32)n, id) == linear_find(ids, id));
      };
      probe(0);
      probe(1);
      probe(0xFFFFFFFFu);
      for (size_t i = 0; i < n; i++) {
        probe(ids[i].id);      // present (the first and the last among them)
        probe(ids[i].id - 1);  // the gap below (or the neighbour, where there is none)
        probe(ids[i].id + 1);  // the gap above
        if (i + 1 < n) probe(ids[i].id + (ids[i + 1].id - ids[i].id) / 2);
      }
      for (size_t i = 0; i < n; i++) CHECK(zh_dictset_find(ids.data(), (u32)n, ids[i].id) == (int32_t)ids[i].index);
    }
  return probes;
}

static void check_creation() {
  snprintf(g_where, sizeof g_where, "creation");
  u32 n_out = 99;
  {  // unsorted IDs with raw-content entries in between
    const u32 raw[] = {700, 0, 5, 0xFFFFFFFFu, 0, 1, 0, 42};
    std::vector<ZhDictSetId> out(8);
    CHECK(zh_dictset_sort_ids(raw, 8, out.data(), &n_out) && n_out == 5);
    const u32 want_id[] = {1, 5, 42, 700, 0xFFFFFFFFu}, want_ix[] = {5, 2, 7, 0, 3};
    for (u32 i = 0; i < 5 && i < n_out; i++) CHECK(out[i].id == want_id[i] && out[i].index == want_ix[i]);
    for (u32 i = 0; i < 8; i++) CHECK(zh_dictset_find(out.data(), n_out, raw[i]) == (raw[i] ? (int32_t)i : -1));
  }
  {  // only raw content: accepted, nothing to find
    const u32 raw[] = {0, 0, 0};
    std::vector<ZhDictSetId> out(3);
    CHECK(zh_dictset_sort_ids(raw, 3, out.data(), &n_out) && n_out == 0);
  }
  {  // a shared non-zero ID, adjacent or far apart
    const u32 a[] = {9, 9}, b[] = {3, 0, 8, 1, 0, 3};
    std::vector<ZhDictSetId> out(6);
    CHECK(!zh_dictset_sort_ids(a, 2, out.data(), &n_out) && n_out == 0);
    CHECK(!zh_dictset_sort_ids(b, 6, out.data(), &n_out) && n_out == 0);
  }
  {  // the count's bounds; a full set of distinct IDs in descending order, and one with a duplicate at the end
    std::vector<u32> raw(ZH_DICTSET_MAX + 1);
    std::vector<ZhDictSetId> out(ZH_DICTSET_MAX + 1);
    for (u32 i = 0; i <= ZH_DICTSET_MAX; i++) raw[i] = 3u * (ZH_DICTSET_MAX + 1 - i);
    CHECK(!zh_dictset_sort_ids(raw.data(), 0, out.data(), &n_out));
    CHECK(!zh_dictset_sort_ids(raw.data(), ZH_DICTSET_MAX + 1, out.data(), &n_out));
    CHECK(zh_dictset_sort_ids(raw.data(), ZH_DICTSET_MAX, out.data(), &n_out) && n_out == ZH_DICTSET_MAX);
    for (u32 i = 1; i < n_out; i++) CHECK(out[i - 1].id < out[i].id);
    for (u32 i = 0; i < ZH_DICTSET_MAX; i += 97) CHECK(zh_dictset_find(out.data(), n_out, raw[i]) == (int32_t)i);
    raw[ZH_DICTSET_MAX - 1] = raw[0];
    CHECK(!zh_dictset_sort_ids(raw.data(), ZH_DICTSET_MAX, out.data(), &n_out));
  }
}

static bool same_desc(const ZhBlockDesc &a, const ZhBlockDesc &b) {
  return a.src == b.src && a.dst == b.dst && a.frame_size == b.frame_size && a.n == b.n && a.item == b.item && a.dst_cap == b.dst_cap &&
         a.flags == b.flags && a.pre == b.pre && a.pre_n == b.pre_n && a.dict_id == b.dict_id;
}
static bool same_item(const ZhItemDesc &a, const ZhItemDesc &b) {
  return a.dst == b.dst && a.cap == b.cap && a.first_block == b.first_block && a.nblocks == b.nblocks;
}

static long check_rule() {
  const u64 sizes[] = {1, 32767, 32768, 32769, 65536};
  const int levels[] = {1, 3, 5};
  const u32 contents[] = {256, 511, 512, 65535, 65536, 131072};
  const u32 first_slot = 7, index = 3, off = 40;  // (entries 0, 2, 4: formatted, content after `off` bytes)
  std::vector<u8> src(65536), out(16), staging((size_t)(first_slot + 8) * ZH_STAGE_SLOT);
  // the set: one entry per content length, IDs 0 (raw) and non-zero alternating; a blob pointer on
  // the formatted ones (never dereferenced here)
  std::vector<std::vector<u8>> bufs;
  std::vector<ZhDictSetEntry> ents;
  static const int blob_tag = 0;
  for (u32 c : contents) {
    bool const fmt = ents.size() % 2 == 0;
    bufs.emplace_back((size_t)c + (fmt ? off : 0u));
    ZhDictSetEntry e{};
    e.buf = bufs.back().data();
    e.n = (u32)bufs.back().size();
    e.off = fmt ? off : 0u;
    e.id = fmt ? 0x1000u + (u32)ents.size() : 0u;
    e.dent = fmt ? (const ZhDictEnt *)&blob_tag : nullptr;
    ents.push_back(e);
  }
  u32 const count = (u32)ents.size();
  long walked = 0;
  for (u64 size : sizes)
    for (int level : levels)
      for (u32 e = 0; e < count; e++)
        for (u32 dent = 0; dent < 2; dent++)
          for (u32 extra = 0; extra < 4; extra += 3) {
            snprintf(g_where, sizeof g_where, "size %llu level %d entry %u dict_entropy %u extra %u", (unsigned long long)size, level, e, dent,
                     extra);
            ZhBatchPlan p{};  // the set batch: no batch dictionary
            p.flags = ZH_F_CHECKSUM;
            p.hist = level >= 3;
            p.staging = staging.data();
            p.out_cap = 1u << 20;
            ZhBatchPlan q = p;  // the batch of a handle with that one dictionary set
            q.dict = ents[e].buf + ents[e].off;
            q.dict_n = ents[e].n - ents[e].off;
            q.dict_id = ents[e].id;
            if (dent && ents[e].dent) q.flags |= ZH_F_DICTENT;
            ZhPlanItem const plain{src.data(), size, index, level, out.data()};
            ZhPlanItem with = plain;
            zh_dictset_plan_item(with, ents.data(), count, (int32_t)e, dent != 0);
            bool inv_a = true, inv_b = true;
            ZhItemDesc const ia = zh_item_desc(p, with, first_slot, &inv_a), ib = zh_item_desc(q, plain, first_slot, &inv_b);
            CHECK(!inv_a && !inv_b && same_item(ia, ib));
            u32 const bpi = (u32)zh_frame_blocks(size, zh_split_dict(level, true)) + extra;
            CHECK(ia.nblocks <= bpi && bpi <= 8);
            for (u32 k = 0; k < bpi; k++) {
              ZhBlockDesc const a = zh_block_desc(p, with, k, first_slot + k), b = zh_block_desc(q, plain, k, first_slot + k);
              walked++;
              CHECK(same_desc(a, b));
              CHECK((a.flags & ZH_F_DICT) && a.dict_id == ents[e].id);
              CHECK(!!(a.flags & ZH_F_DICTENT) == (dent && ents[e].dent != nullptr));
              CHECK((a.n == 0) == (k >= ia.nblocks));
              if (k == 0) CHECK(a.pre + a.pre_n == ents[e].buf + ents[e].n && a.pre_n <= ents[e].n - ents[e].off);
            }
            // index -1: the descriptors of a dictionary-less batch, padded to the set batch's blocks per item
            ZhPlanItem none = plain;
            none.pre = src.data(), none.pre_n = 77, none.dict_id = 5, none.flags = ZH_F_DICTENT;  // (all reset)
            zh_dictset_plan_item(none, ents.data(), count, -1, dent != 0);
            bool inv_n = true, inv_p = true;
            ZhItemDesc const in = zh_item_desc(p, none, first_slot, &inv_n), ip = zh_item_desc(p, plain, first_slot, &inv_p);
            CHECK(!inv_n && !inv_p && same_item(in, ip) && in.nblocks == zh_frame_blocks(size, false) && in.nblocks <= bpi);
            for (u32 k = 0; k < bpi; k++) {
              ZhBlockDesc const a = zh_block_desc(p, none, k, first_slot + k), b = zh_block_desc(p, plain, k, first_slot + k);
              walked++;
              CHECK(same_desc(a, b) && !(a.flags & (ZH_F_DICT | ZH_F_DICTENT)) && a.dict_id == 0 && (a.n == 0) == (k >= in.nblocks));
              if (k == 0) CHECK(a.pre == nullptr && a.pre_n == 0);
            }
            // a bad index: every slot inactive, the item invalid
            for (int32_t bad : {-2, (int32_t)count, (int32_t)0x7FFFFFFF, (int32_t)0x80000000}) {
              ZhPlanItem b = plain;
              zh_dictset_plan_item(b, ents.data(), count, bad, dent != 0);
              bool invalid = false;
              (void)zh_item_desc(p, b, first_slot, &invalid);
              CHECK(invalid);
              for (u32 k = 0; k < bpi; k++) {
                walked++;
                CHECK(zh_block_desc(p, b, k, first_slot + k).n == 0);
              }
            }
          }
  return walked;
}

int main() {
  long const a = check_find();
  check_creation();
  long const b = check_rule();
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("dictset OK (%ld lookups, %ld descriptors)\n", a, b);
  return 0;
}

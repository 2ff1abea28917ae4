// zh_dictset.h — a set of dictionaries on the device: the entry table the plan and the stages read,
// the Dictionary_ID lookup, the validation and sort done at creation, and the step that turns an
// item's entry index into the descriptor rule's input (zh_block_plan.h).  Plain C++, no HIP types:
// tests/cpp/dictset_check.cpp walks all of it on the host.
#pragma once
#include "zh_block_plan.h"

struct ZhDictEnt;

// Most dictionaries in one set.  Device bytes per entry, all in the set's one allocation: the
// dictionary buffer (256 B .. 128 KiB), K1's packed tables (64 KiB, entries with >= 512 content
// bytes), the deep matcher's links (4 B per staged content byte, <= 256 KiB) and head table
// (64 KiB), a formatted dictionary's entropy blob (sizeof(ZhDictEnt), ~6.5 KiB), this record and 8 B
// of the ID array: ~0.5 MiB for a 64 KiB dictionary, 2 GiB for a full set of them.
#define ZH_DICTSET_MAX 4096u

// One entry: all the device state of one dictionary.  A handle's own dictionary is the entry of a
// set of one; a view of caller memory is buf and n alone, the rest 0 (zh_host.cpp DevDict).
struct ZhDictSetEntry {
  const u8 *buf;        // the whole buffer (the decoder reads a formatted dictionary's tables from it)
  u32 n, off, id;       // its size, content offset and Dictionary_ID (0: raw content)
  u32 dtab_P;           // K1's tables cover the last dtab_P content bytes (0: none)
  const u16 *dtab;      // K1's packed tables (ZhWorkspace::dtab)
  const u32 *dd_prev;   // the deep matcher's chains (ZhWorkspace::dd_*; dd_pre 0: none)
  const u32 *dd_head;
  u32 dd_pre, dd_split;
  const ZhDictEnt *dent;  // the entropy blob of a formatted dictionary the encoder can use, else null
};

// The non-zero IDs of a set, sorted, with their entry indices
struct ZhDictSetId {
  u32 id, index;
};

// Entry index of Dictionary_ID `id` in the sorted array, or -1 (id 0 is never found: raw-content
// entries are reachable by index only)
ZH_BP_HD int32_t zh_dictset_find(const ZhDictSetId *ids, u32 n, u32 id) {
  if (id == 0) return -1;
  u32 lo = 0, hi = n;
  while (lo < hi) {
    u32 const mid = lo + (hi - lo) / 2;
    if (ids[mid].id < id) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && ids[lo].id == id ? (int32_t)ids[lo].index : -1;
}

// Creation: out (room for n) = the non-zero IDs of ids[0, n) sorted with their indices, *n_out how
// many.  false: n outside 1 .. ZH_DICTSET_MAX, or two entries share a non-zero ID.  (A heap sort:
// no allocation, no recursion, usable wherever this header is.)
inline bool zh_dictset_sort_ids(const u32 *ids, size_t n, ZhDictSetId *out, u32 *n_out) {
  *n_out = 0;
  if (n < 1 || n > ZH_DICTSET_MAX) return false;
  u32 m = 0;
  for (size_t i = 0; i < n; i++)
    if (ids[i]) out[m++] = ZhDictSetId{ids[i], (u32)i};
  auto sift = [out](u32 root, u32 end) {
    for (;;) {
      u32 c = 2 * root + 1;
      if (c >= end) return;
      if (c + 1 < end && out[c].id < out[c + 1].id) c++;
      if (out[root].id >= out[c].id) return;
      ZhDictSetId const t = out[root];
      out[root] = out[c];
      out[c] = t;
      root = c;
    }
  };
  for (u32 i = m / 2; i-- > 0;) sift(i, m);
  for (u32 end = m; end > 1; end--) {
    ZhDictSetId const t = out[0];
    out[0] = out[end - 1];
    out[end - 1] = t;
    sift(0, end - 1);
  }
  for (u32 i = 1; i < m; i++)
    if (out[i].id == out[i - 1].id) return false;
  *n_out = m;
  return true;
}

// A set-route item: `it` (src, size, index, level, out filled) planned against entry idx of
// ents[0, count).  idx >= 0: the entry's content is the item's prefix and its ID the frames'
// Dictionary_ID, with ZH_F_DICTENT when the set asks for entropy sections and the entry has a
// usable one; -1: no dictionary; anything else: a prefix length without a pointer, which the rule
// turns into inactive slots and an invalid item.
ZH_BP_HD void zh_dictset_plan_item(ZhPlanItem &it, const ZhDictSetEntry *ents, u32 count, int32_t idx, bool dict_entropy) {
  it.pre = nullptr;
  it.pre_n = 0;
  it.dict_id = 0;
  it.flags = 0;
  if (idx == -1) return;
  if (idx < -1 || (u32)idx >= count) { it.pre_n = 1; return; }
  ZhDictSetEntry const &e = ents[idx];
  it.pre = e.buf + e.off;
  it.pre_n = e.n - e.off;
  it.dict_id = e.id;
  it.flags = dict_entropy && e.dent ? (u32)ZH_F_DICTENT : 0u;
}

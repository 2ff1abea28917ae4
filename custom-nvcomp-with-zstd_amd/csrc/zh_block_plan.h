// zh_block_plan.h — the block descriptors of a frame: the one rule behind the host plan
// (ZstdBatchManager::Impl::run, zh_host.cpp) and the two device plans (zh_plan_kernel,
// zh_plan_levels_kernel, zh_plan.hip).  Plain C++, no HIP types: tests/cpp/block_plan_check.cpp
// and tests/cpp/prefix_plan_check.cpp (the per-item prefix) walk the rule on the host, as does
// tests/cpp/dictset_check.cpp for an item of a dictionary-set batch (zh_dictset.h).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "zstd_hip_params.h"

#if defined(__HIPCC__)
#define ZH_BP_HD __host__ __device__ inline
#else
#define ZH_BP_HD inline
#endif

typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;

// One device block (<= ZH_BLOCK_MAX input bytes) = one K1 workgroup = one K2 wave.
struct ZhBlockDesc {
  const u8 *src;     // first input byte of this block
  u8 *dst;           // where this block's output goes (item output if DIRECT, else staging slot)
  u64 frame_size;    // content size of the frame this block belongs to
  u32 n;             // input bytes (0 = inactive slot)
  u32 item;          // batch item index
  u32 dst_cap;       // bytes available at dst
  u32 flags;         // ZH_F_* below
  const u8 *pre;     // staged before the block: a ZH_F_DICT first block's content tail, a later block's previous ZH_HIST_BLOCK bytes
  u32 pre_n;         // its length (pre_n + n <= ZH_BLOCK_MAX; ZH_F_DEEP: pre_n <= ZH_DEEP_PRE), 0 without one
  u32 dict_id;       // Dictionary_ID written to the frame header (0: none)
};

enum : u32 {
  ZH_F_FIRST = 1u,   // first block of its frame: writes the frame header, starts with reps {1,4,8}
  ZH_F_LAST = 2u,    // last block of its frame: Last_Block bit
  ZH_F_DIRECT = 4u,  // single-block frame written straight into the item's output
  ZH_F_CHECKSUM = 8u,  // frame carries a content checksum (first block: FHD bit; zh_checksum_kernel appends it)
  ZH_F_DICT = 16u,     // dictionary frame: Dictionary_ID in the header, repcodes start unknown
  ZH_F_DEEP = 32u,     // level >= ZH_DEEP_LEVEL (zh_lz_deep.hip): a dictionary frame's first block is staged
                       // behind the last ZH_DEEP_PRE content bytes
  ZH_F_LDM = 64u,      // one-sequence block of a long-distance match (zh_ldm.hip): n = 0, so K1-K4 skip the slot; its
                       // bytes and staged size are already written, and the gather copies them like any block's
  ZH_F_DICTENT = 128u, // CompressionConfig::dict_entropy with a formatted dictionary (ZhWorkspace::dent): the first
                       // block of a frame starts from the dictionary's repcodes and may reuse its entropy tables
                       // (treeless literals, Repeat_Mode sequence tables)
  ZH_F_STATS = 256u,   // statistics pass of dictionary finalisation: the entropy kernel adds every block's literal
                       // histogram and LL / OF / ML code counts to ZhWorkspace::stats (integer atomics)
};

// Per-item bookkeeping for frames that span several device blocks.
struct ZhItemDesc {
  u8 *dst;           // item output
  u64 cap;           // item output capacity
  u32 first_block;   // index of the item's first ZhBlockDesc
  u32 nblocks;       // number of device blocks in the frame
};

// Staging slot for one block of a multi-block frame: worst case = raw block + frame header.
#define ZH_STAGE_SLOT ((u32)ZH_BLOCK_MAX + 64u)

// Status codes written per item (values of cuda_zstd::Status).
enum : u32 { ZH_ST_OK = 0, ZH_ST_INVALID = 2, ZH_ST_TOO_SMALL = 7 };

// What is constant over one batch.
struct ZhBatchPlan {
  u32 flags;       // frame flags every block carries: ZH_F_CHECKSUM, ZH_F_DICTENT, ZH_F_STATS
  u32 hist;        // the frames' window reaches the previous block (ZH_HIST_WINDOW_LOG)
  const u8 *dict;  // dictionary content (null: none), its length and Dictionary_ID
  u32 dict_n, dict_id;
  u8 *staging;     // ZH_STAGE_SLOT bytes per block slot (multi-block frames)
  u64 out_cap;     // output capacity: one for the batch (device plans), set per item by the host plan
};

// One item of the batch.  pre / pre_n: the item's own prefix (pre_n 0: none), the bytes that
// precede the chunk as a raw-content dictionary without a Dictionary_ID; the item then gets the
// descriptors of a batch whose dictionary is that prefix, an item without one those of a
// dictionary-less frame.  Not together with ZhBatchPlan::dict.  dict_id / flags: an item of a
// dictionary-set batch (zh_dictset.h) is planned behind its entry's content, and its frames carry
// that entry's Dictionary_ID and frame flags (ZH_F_DICTENT).
struct ZhPlanItem {
  const u8 *src;
  u64 size;
  u32 index;
  int level;
  u8 *out;
  const u8 *pre = nullptr;
  u64 pre_n = 0;
  u32 dict_id = 0;
  u32 flags = 0;
};

// A dictionary frame below ZH_DEEP_LEVEL is cut into 32 KiB blocks from 32 KiB on (ZH_FRAME_BLOCK)
ZH_BP_HD bool zh_split_dict(int level, bool has_dict) { return has_dict && level < ZH_DEEP_LEVEL; }
ZH_BP_HD u64 zh_frame_blocks(u64 size, bool split_dict) {
  u64 const bs = ZH_FRAME_BLOCK(size, split_dict);
  return (size + bs - 1) / bs;
}

// Block k of item `it`, written to block slot `slot` (k at or past the frame's block count: an
// inactive padding slot, n = 0).
// The item's prefix source: the batch's dictionary, or the item's own prefix
ZH_BP_HD bool zh_item_has_dict(const ZhBatchPlan &p, const ZhPlanItem &it) { return p.dict != nullptr || it.pre_n != 0; }
// An item that names a prefix length without a pointer has no frame
ZH_BP_HD bool zh_item_bad_prefix(const ZhBatchPlan &p, const ZhPlanItem &it) { return !p.dict && it.pre_n != 0 && it.pre == nullptr; }

ZH_BP_HD ZhBlockDesc zh_block_desc(const ZhBatchPlan &p, const ZhPlanItem &it, u32 k, u32 slot) {
  bool const has_dict = zh_item_has_dict(p, it);
  bool const deep = it.level >= ZH_DEEP_LEVEL, split = zh_split_dict(it.level, has_dict);
  u64 const bs = ZH_FRAME_BLOCK(it.size, split), nb = zh_frame_blocks(it.size, split);
  ZhBlockDesc d;
  d.src = it.src + (u64)k * bs;
  d.frame_size = it.size;
  d.item = it.index;
  d.n = 0;
  if (k < nb && !zh_item_bad_prefix(p, it)) d.n = (u32)(it.size - (u64)k * bs < bs ? it.size - (u64)k * bs : bs);
  d.flags = (k == 0 ? ZH_F_FIRST : 0u) | (k + 1 == nb ? ZH_F_LAST : 0u) | (nb == 1 ? ZH_F_DIRECT : 0u) | p.flags | it.flags | (deep ? ZH_F_DEEP : 0u);
  d.pre = nullptr;
  d.pre_n = 0;
  d.dict_id = 0;
  if (k > 0 && p.hist) {  // history frame: the previous 32 KiB block is staged in front
    d.pre = d.src - ZH_HIST_BLOCK;
    d.pre_n = ZH_HIST_BLOCK;
  }
  if (has_dict) {  // dictionary frame: the first block is compressed behind the content's tail
    const u8 *const dict = p.dict ? p.dict : it.pre;
    u64 const dict_n = p.dict ? (u64)p.dict_n : it.pre_n;
    d.flags |= ZH_F_DICT;
    d.dict_id = p.dict ? p.dict_id : it.dict_id;
    if (k == 0) {
      // what fits in front of the block in K1's 64 KiB of LDS; the deep matcher keeps its staged
      // bytes in global memory and takes up to ZH_DEEP_PRE
      u32 const room = deep ? (u32)ZH_DEEP_PRE : (u32)ZH_BLOCK_MAX - d.n;
      d.pre_n = dict_n < room ? (u32)dict_n : room;
      d.pre = dict ? dict + dict_n - d.pre_n : nullptr;
    }
  }
  if (nb == 1) {
    d.dst = it.out;
    d.dst_cap = (u32)(p.out_cap < 0xFFFFFFFFull ? p.out_cap : 0xFFFFFFFFull);
  } else {
    d.dst = p.staging + (size_t)slot * ZH_STAGE_SLOT;
    d.dst_cap = ZH_STAGE_SLOT;
  }
  return d;
}

// The item's descriptor, its blocks starting at block slot first_slot; *invalid: the item has no
// frame (size 0, or a prefix length without a pointer: item size 0, status ZH_ST_INVALID, every
// slot inactive).
ZH_BP_HD ZhItemDesc zh_item_desc(const ZhBatchPlan &p, const ZhPlanItem &it, u32 first_slot, bool *invalid) {
  ZhItemDesc id;
  id.dst = it.out;
  id.cap = p.out_cap;
  id.first_block = first_slot;
  id.nblocks = (u32)zh_frame_blocks(it.size, zh_split_dict(it.level, zh_item_has_dict(p, it)));
  *invalid = it.size == 0 || zh_item_bad_prefix(p, it);
  return id;
}

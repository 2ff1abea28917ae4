// zh_launch.h — host-side entry points into the device pipeline (K1 lz, K2 entropy, K3 gather).
#pragma once
#include "zh_common.h"
#include "zh_ldm.h"

// Per-item bookkeeping for frames that span several device blocks.
struct ZhItemDesc {
  u8 *dst;           // item output
  u64 cap;           // item output capacity
  u32 first_block;   // index of the item's first ZhBlockDesc
  u32 nblocks;       // number of device blocks in the frame
};

// Staging slot for one block of a multi-block frame: worst case = raw block + frame header.
#define ZH_STAGE_SLOT ((u32)ZH_BLOCK_MAX + 64u)

// Decoder launch (zh_decode.hip): one workgroup per input buffer; every array is a
// device array indexed by item.  Item i's workspace slot is ws + i * slot_bytes:
// block_cap literal bytes (padded to lit_bytes), then seq_cap u64 sequence records.
struct ZhDecArgs {
  const void *const *in_ptrs;  // null: a single item given by one_in / one_in_size / one_out
  const void *one_in;
  u64 one_in_size;
  void *one_out;
  const size_t *in_sizes;
  void *const *out_ptrs;
  const size_t *out_caps;  // per-item output capacity, or null: out_cap_all for every item
  u64 out_cap_all;
  size_t *out_sizes;       // bytes produced (0 on error)
  u32 *statuses;           // optional: Status values, or nvcomp codes when nvcomp_codes
  u8 *ws;
  u64 slot_bytes;
  u32 lit_bytes, block_cap, seq_cap, nvcomp_codes;
  u32 ho_off;  // offset of the item's hand-off record (deferred buffers) inside its slot
  const u8 *dict;  // dictionary (device, whole buffer) or null; its content precedes every frame
  u64 dict_n;      // its size
  u32 dict_off;    // content offset (formatted dictionary: after tables + repcodes; raw: 0)
  u32 dict_id;     // Dictionary_ID (formatted), 0 for raw content
};
#define ZH_DEC_HANDOFF_BYTES 5376u  // sizeof(DecHandoff), zh_decode.hip

namespace zh {
u32 dec_lds_bytes();
// Walker (one pass; from 2,048 items a tables and a rest pass), sequence kernel, execution kernel.
hipError_t launch_decompress(const ZhDecArgs &a, u32 nitems, hipStream_t stream);
// Size pass of the walker: out_sizes[i] = the bytes item i's frames regenerate (exact with or without
// a Frame_Content_Size), statuses[i] (optional) as in decode.  Reads in_ptrs / in_sizes (or one_in),
// the dictionary fields and nvcomp_codes; no workspace, no output pointers.  One launch, no sync.
hipError_t launch_decompress_sizes(const ZhDecArgs &a, u32 nitems, hipStream_t stream);
hipError_t init_kernels();
u32 lz_lds_bytes();
u32 entropy_lds_bytes();
// K1 hash tables of a dictionary's content tail, built once per dictionary (zh_lz.hip):
// out = 2^15 u16, tmp32 = 2^15 u32 scratch; P = the tail length covered (0: none)
hipError_t lz_dict_tables(const u8 *content, size_t cn, u16 *out, u32 *tmp32, u32 &P, hipStream_t stream);
hipError_t lz_deep_dict_tables(const u8 *content, size_t cn, u8 *stg, u32 *dprev, u32 *dhead, u32 &P, u32 &split, hipStream_t stream);
hipError_t launch_compress(const ZhBlockDesc *d_descs, u32 nblocks, ZhWorkspace ws, u32 window_log, u32 cfg_block_size, u64 *d_item_size,
                           u32 *d_item_status, u32 *d_blk_size, const ZhItemDesc *d_items, u32 nitems, bool gather, bool checksum, int level,
                           hipStream_t stream);
void profile_enable(bool on);
int profile_collect(double *totals);
hipError_t launch_plan(const void *const *d_in_ptrs, const size_t *d_in_sizes, u32 nitems, u32 bpi, void *const *d_out_ptrs, u64 out_cap,
                       u8 *staging, ZhBlockDesc *d_descs, ZhItemDesc *d_items, u64 *d_item_size, u32 *d_item_status, u32 extra_flags,
                       const u8 *dict, u32 dict_n, u32 dict_id, u32 hist, hipStream_t stream);
// Mixed-level batch (zh_plan.hip): d_levels[i] = item i's level, a device array.  launch_plan_levels
// ranks the items by parse class (one workgroup, up to ZH_RANK_MAX_ITEMS items) and writes the
// descriptors at their sorted slots with one level byte per slot; launch_compress_levels runs the
// matchers over the class ranges left in *d_ranges, then the same entropy / gather / checksum stages.
#define ZH_RANK_MAX_ITEMS (1u << 20)
hipError_t launch_plan_levels(const void *const *d_in_ptrs, const size_t *d_in_sizes, const int *d_levels, u32 nitems, u32 bpi,
                              void *const *d_out_ptrs, u64 out_cap, u8 *staging, ZhBlockDesc *d_descs, u8 *d_blk_level, u32 *d_rank,
                              ZhClassRanges *d_ranges, ZhItemDesc *d_items, u64 *d_item_size, u32 *d_item_status, u32 extra_flags,
                              hipStream_t stream);
hipError_t launch_compress_levels(const ZhBlockDesc *d_descs, u32 nblocks, ZhWorkspace ws, u32 cfg_block_size, u64 *d_item_size,
                                  u32 *d_item_status, u32 *d_blk_size, const ZhItemDesc *d_items, u32 nitems, bool gather, bool checksum,
                                  ZhClassRanges *d_ranges, const u8 *d_blk_level, hipStream_t stream);
// Long-distance matching (zh_ldm.hip): index + per-cell split of one frame, three descriptor slots per cell
hipError_t ldm_launch(const u8 *src, u64 size, u32 ncells, u32 table_log, u32 max_dist, u32 flags, u64 *table, u64 *skey, u32 *sslot,
                      u32 *scount, ZhBlockDesc *descs, u8 *staging, u32 *blk_size, ZhLdmRecord *rec, hipStream_t stream);
double ldm_profile(bool on);
}  // namespace zh

// zh_launch.h — host-side entry points into the device pipeline (K1 lz, K2 entropy, K3 gather).
#pragma once
#include "zh_common.h"
#include "zh_ldm.h"

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
  // one prefix per item (device arrays, or null: none): raw content in front of item i's frames,
  // all of it addressable; not together with dict.  A zero size or a null pointer: no prefix
  const void *const *pre_ptrs;
  const size_t *pre_sizes;
  // a dictionary set (zh_dictset.h; null: none; not together with dict or prefixes): every frame's
  // dictionary is resolved on the device, from its Dictionary_ID over set_ids[0, set_nids) or, where
  // dict_index (optional, per item) is >= 0, that entry of set[0, set_count)
  const ZhDictSetEntry *set;
  const ZhDictSetId *set_ids;
  const int32_t *dict_index;
  u32 set_count, set_nids;
};
#define ZH_DEC_HANDOFF_BYTES 5376u  // sizeof(DecHandoff), zh_decode.hip

// One batch bound to its workspace (zh_host.cpp bind_batch): where the plan (launch_plan, or the
// host's upload) writes and the stages (launch_compress) read.
struct ZhBatch {
  ZhBlockDesc *descs;  // nblocks block slots
  ZhItemDesc *items;   // nitems
  u64 *item_size;      // per item: the frame's bytes
  u32 *item_status;    // per item: ZH_ST_*
  u32 *blk_size;       // per block slot: staged bytes of a multi-block frame's block
  ZhBatchPlan plan;    // the descriptor rule's batch constants (zh_block_plan.h), staging included
  ZhWorkspace ws;
  u32 *rank;              // a mixed-level batch (null otherwise): the items' ranks,
  u8 *blk_level;          // one level byte per block slot,
  ZhClassRanges *ranges;  // the class ranges with the matchers' counters
  u32 nblocks, nitems;
  u32 window_log, block_size;  // the frames' window descriptor (mixed-level: per block, from blk_level) and block size
  int level;                   // every item's level (not read for a mixed-level batch)
  bool gather, checksum;       // multi-block frames to concatenate; content checksums to append
};

// The device arrays launch_plan reads: the items' inputs and outputs
struct ZhPlanArrays {
  const void *const *in_ptrs;
  const size_t *in_sizes;
  void *const *out_ptrs;
  const int *levels;  // one level per item (a mixed-level batch), or null
  // one prefix per item (ZhPlanItem::pre / pre_n), or both null; prefix_sizes[i] == 0: item i has none
  const void *const *prefix_ptrs;
  const size_t *prefix_sizes;
  // one entry of a dictionary set per item (zh_dictset.h), or null: dict_index[i] names an entry of
  // set[0, set_count), -1 none; set_entropy: the handle's dict_entropy setting
  const int32_t *dict_index;
  const ZhDictSetEntry *set;
  u32 set_count, set_entropy;
};

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
// A dictionary's precomputed tables, built once per dictionary with the dictionary as a grid
// dimension (one job for a handle's own dictionary, a group for a dictionary set): K1's hash tables
// of the content tail (zh_lz.hip) and the deep matcher's chains (zh_lz_deep.hip) of d_jobs[0, count)
// in one memset and three launches whatever count is.  tmp32: count x 2^15 u32, stg: count x
// ZH_DEEP_DICT_STG bytes of scratch.  lz_dict_tables_P / lz_deep_dict_shape: the tail length P (and
// split) the builders cover for cn content bytes (0: none), from which the caller fills the jobs.
u32 lz_dict_tables_P(size_t cn);
void lz_deep_dict_shape(size_t cn, u32 &P, u32 &split);
hipError_t lz_dict_tables_batch(const ZhDictBuildJob *d_jobs, u32 count, u32 *tmp32, hipStream_t stream);
hipError_t lz_deep_dict_tables_batch(const ZhDictBuildJob *d_jobs, u32 count, u8 *stg, hipStream_t stream);
// The stages of one batch: the matchers (ranges null: every block at b.level; else the class ranges
// the rank kernel left in *b.ranges), entropy, gather, checksum.
hipError_t launch_compress(const ZhBatch &b, hipStream_t stream);
void profile_enable(bool on);
int profile_collect(double *totals);
// Device plan (zh_plan.hip): descs, items and the invalid items' size and status from the device
// arrays in `a`; every item takes nblocks / nitems block slots.  a.levels (a mixed-level batch):
// the items are ranked by parse class (one workgroup, up to ZH_RANK_MAX_ITEMS items) and their
// descriptors written at the sorted slots with one level byte per slot.  a.prefix_sizes: item i is
// planned behind its own prefix (a.prefix_ptrs[i], a.prefix_sizes[i] bytes; 0: none).
#define ZH_RANK_MAX_ITEMS (1u << 20)
hipError_t launch_plan(const ZhBatch &b, const ZhPlanArrays &a, hipStream_t stream);
// Long-distance matching (zh_ldm.hip): index + per-cell split of one frame, three descriptor slots per cell
hipError_t ldm_launch(const u8 *src, u64 size, u32 ncells, u32 table_log, u32 max_dist, u32 flags, u64 *table, u64 *skey, u32 *sslot,
                      u32 *scount, ZhBlockDesc *descs, u8 *staging, u32 *blk_size, ZhLdmRecord *rec, hipStream_t stream);
double ldm_profile(bool on);
// Many streams (zh_stream.hip): stream i's window pair is windows + i * 2 * ZH_STREAM_WINDOW, which[i]
// its current half, pre_ptrs[i] / pre_sizes[i] the current window as the batch entries' prefix.
// window_update_launch: one workgroup per stream appends chunk i (chunk_sizes[i] bytes; statuses[i]
// non-zero or no bytes: the window stays) and writes the stream's next prefix pointer and size.
hipError_t window_update_launch(u8 *windows, u32 *which, const void **pre_ptrs, size_t *pre_sizes, const void *const *chunk_ptrs,
                                const size_t *chunk_sizes, const u32 *statuses, u32 nstreams, hipStream_t stream);
double window_profile(bool on);
hipError_t window_reset_launch(u8 *windows, u32 *which, const void **pre_ptrs, size_t *pre_sizes, u32 nstreams, hipStream_t stream);
}  // namespace zh

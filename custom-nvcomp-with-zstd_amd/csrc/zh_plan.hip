// zh_plan.hip — batch planning, multi-block frame gather, and launch wrappers.
//
// zh_plan_kernel : builds one ZhBlockDesc per (item, block slot) from device pointer/size
//                  arrays with the rule of zh_block_plan.h, for the stream-ordered batched
//                  entry points (no host round trip, unlike the reference's compress_async,
//                  src/cuda_zstd_nvcomp.cpp:319-437); zh_plan_levels_kernel: one level per item.
//                  With ZhPlanArrays::prefix_ptrs / prefix_sizes every item brings its own prefix
//                  (the bytes in front of it, a raw-content dictionary): ZhPlanItem::pre / pre_n.
//                  With ZhPlanArrays::dict_index every item names an entry of a dictionary set
//                  (zh_dictset.h): that entry's content, Dictionary_ID and frame flags.
// zh_gather_kernel: concatenates the staged blocks of multi-block frames (the
//                  reference assembles them on the host with blocking copies,
//                  src/cuda_zstd_manager.cu:2765-3027).
#include "zh_common.h"
#include "zh_launch.h"
#include "zh_scan.h"
#include "zh_xxh64.h"

#include <mutex>
#include <vector>

extern "C" u32 zh_lz_lds_bytes();
extern "C" u32 zh_entropy_lds_bytes();
namespace zh {
hipError_t lz_init();
void lz_launch(const ZhBlockDesc *d_descs, u32 nblocks, ZhWorkspace ws, u32 mode, hipStream_t stream);
void lz_launch_ranged(const ZhBlockDesc *d_descs, u32 nblocks, ZhWorkspace ws, ZhClassRanges *d_ranges, hipStream_t stream);
hipError_t lz_deep_init();
hipError_t lz_deep_launch(const ZhBlockDesc *d_descs, u32 nblocks, ZhWorkspace ws, int level, hipStream_t stream);
hipError_t lz_deep_launch_ranged(const ZhBlockDesc *d_descs, u32 nblocks, ZhWorkspace ws, ZhClassRanges *d_ranges, const u8 *d_blk_level,
                                 hipStream_t stream);
hipError_t entropy_init();
void entropy_launch(const ZhBlockDesc *d_descs, u32 nblocks, ZhWorkspace ws, u32 window_log, u32 cfg_block_size, u64 *d_item_size,
                    u32 *d_item_status, u32 *d_blk_size, const u8 *d_blk_level, hipStream_t stream);
}  // namespace zh

// The device plans: thread t is block k = t % bpi of item i = t / bpi, bpi = nblocks / nitems
// slots per item, and writes block slot b with the rule of zh_block_plan.h.  valid false: an
// inactive slot and an invalid item.
__device__ inline void zh_plan_block(const ZhBatch &B, const ZhPlanArrays &a, u32 i, u32 k, u32 b, int level, bool valid) {
  ZhPlanItem it{(const u8 *)a.in_ptrs[i], a.in_sizes[i], i, level, (u8 *)a.out_ptrs[i]};
  if (a.prefix_sizes) { it.pre = (const u8 *)a.prefix_ptrs[i]; it.pre_n = a.prefix_sizes[i]; }  // the item's own prefix
  if (a.dict_index) zh_dictset_plan_item(it, a.set, a.set_count, a.dict_index[i], a.set_entropy != 0);  // its entry of the set
  ZhBlockDesc d = zh_block_desc(B.plan, it, k, b);
  if (!valid) d.n = 0;
  B.descs[b] = d;
  if (k != 0) return;
  bool invalid;
  B.items[i] = zh_item_desc(B.plan, it, b, &invalid);
  if (invalid || !valid) { B.item_size[i] = 0; B.item_status[i] = ZH_ST_INVALID; }
}

// Every item at B.level, slots in item order.
extern "C" __global__ void zh_plan_kernel(ZhBatch B, ZhPlanArrays a) {
  u32 const t = blockIdx.x * blockDim.x + threadIdx.x, bpi = B.nblocks / B.nitems;
  if (t < B.nblocks) zh_plan_block(B, a, t / bpi, t % bpi, t, B.level, true);
}

// ---- mixed-level batch: one level per item, on the device ----------------------
// zh_rank_kernel: a stable counting sort of the items by parse class (ZH_LEVEL_CLASS), one
// workgroup.  Thread t owns the contiguous items [t * per, (t + 1) * per), so thread order is item
// order; it counts its items per class, the counts are scanned across the workgroup (three classes
// packed into one u64 of ZH_RANK_FIELD-bit fields, block_scan_excl64), and a second pass over the
// same items hands out the ranks.  rank[i] = item i's place in the sorted order; cr = every class's
// block range and the matchers' counters preset to their ranges' begins.
#define ZH_RANK_FIELD 21u
#define ZH_RANK_MASK ((1u << ZH_RANK_FIELD) - 1u)
static_assert(ZH_RANK_MAX_ITEMS <= ZH_RANK_MASK, "a class count fits its field");
static_assert(ZH_NCLASSES <= 12, "four packed words of three classes");
extern "C" __global__ __launch_bounds__(ZH_SCAN_THREADS) void zh_rank_kernel(const int *__restrict__ levels, u32 nitems, u32 bpi,
                                                                             u32 *__restrict__ rank, ZhClassRanges *__restrict__ cr) {
  __shared__ u64 lds[4];
  u32 const tid = threadIdx.x;
  u32 const per = (nitems + ZH_SCAN_THREADS - 1) / ZH_SCAN_THREADS;
  u32 const i0 = min(tid * per, nitems), i1 = min(i0 + per, nitems);
  u64 cnt[4] = {0, 0, 0, 0};
  for (u32 i = i0; i < i1; i++) {
    int const lv = levels[i];
    u32 const c = (u32)ZH_LEVEL_CLASS(lv);
    u64 const one = 1ull << (ZH_RANK_FIELD * (c % 3u));
#pragma unroll
    for (u32 w = 0; w < 4; w++) cnt[w] += c / 3u == w ? one : 0ull;
  }
  u64 run[4], tot[4];
#pragma unroll
  for (u32 w = 0; w < 4; w++) run[w] = block_scan_excl64(cnt[w], lds, tot[w]);
  // class begins (in items): every thread derives them from the totals
  u32 begin[ZH_NCLASSES + 1];
  begin[0] = 0;
#pragma unroll
  for (u32 c = 0; c < ZH_NCLASSES; c++) begin[c + 1] = begin[c] + ((u32)(tot[c / 3u] >> (ZH_RANK_FIELD * (c % 3u))) & ZH_RANK_MASK);
#pragma unroll
  for (u32 c = 0; c < ZH_NCLASSES; c++) run[c / 3u] += (u64)begin[c] << (ZH_RANK_FIELD * (c % 3u));  // begin + earlier threads' < nitems
  for (u32 i = i0; i < i1; i++) {
    int const lv = levels[i];
    u32 const c = (u32)ZH_LEVEL_CLASS(lv), sh = ZH_RANK_FIELD * (c % 3u);
    u64 r = 0;
#pragma unroll
    for (u32 w = 0; w < 4; w++) {
      r = c / 3u == w ? run[w] : r;
      run[w] += c / 3u == w ? 1ull << sh : 0ull;
    }
    rank[i] = (u32)(r >> sh) & ZH_RANK_MASK;
  }
  if (tid < ZH_NCLASSES) {
    u32 b0 = 0, b1 = 0;
#pragma unroll
    for (u32 c = 0; c < ZH_NCLASSES; c++) { b0 = tid == c ? begin[c] : b0; b1 = tid == c ? begin[c + 1] : b1; }
    cr->range[tid][0] = b0 * bpi;
    cr->range[tid][1] = b1 * bpi;
    if (tid <= ZH_CLASS_DEEP0) cr->ctr[tid] = b0 * bpi;  // K1 mode 2, 1, 0; the deep range starts at its first class
  }
}

// zh_plan_kernel for a mixed-level batch: item i's level is a.levels[i], and its bpi descriptors go
// to block slots rank[i] * bpi .. (sorted by parse class); d.item stays i -- everything downstream
// of K1 indexes by block and writes results by d.item, so outputs land in input order -- and the
// item's level is stored per block slot.  A level outside 1..22: size 0, status invalid, inactive slots.
extern "C" __global__ void zh_plan_levels_kernel(ZhBatch B, ZhPlanArrays a) {
  u32 const t = blockIdx.x * blockDim.x + threadIdx.x, bpi = B.nblocks / B.nitems;
  if (t >= B.nblocks) return;
  u32 const i = t / bpi, k = t % bpi, b = B.rank[i] * bpi + k;
  int const level = a.levels[i];
  bool const valid = ZH_LEVEL_VALID(level);
  zh_plan_block(B, a, i, k, b, level, valid);
  B.blk_level[b] = valid ? (u8)level : (u8)0;
}
// (a mixed-level batch is bound with plan.hist set whatever the manager's window)
static_assert(ZH_LEVEL_WINDOW_LOG(1) >= ZH_HIST_WINDOW_LOG, "every level's frames may reach the previous block");

// One workgroup per block: a block of a multi-block frame sums the staged sizes of its
// frame's blocks (its output offset and the frame's total), the frame's first block sets the
// item's size and status, and every block copies its own staged bytes (a 64 MiB frame is
// 1024 workgroups, not one).
extern "C" __global__ __launch_bounds__(256) void zh_gather_kernel(const ZhItemDesc *__restrict__ items, const ZhBlockDesc *__restrict__ descs,
                                                                    const u32 *__restrict__ blk_size, u64 *item_size, u32 *item_status) {
  u32 const b = blockIdx.x, tid = threadIdx.x;
  ZhBlockDesc const d = descs[b];
  if (d.n == 0 && !(d.flags & ZH_F_LDM)) return;
  ZhItemDesc const id = items[d.item];
  if (id.nblocks <= 1) return;
  u32 const k = b - id.first_block;
  __shared__ u64 part[2][4];
  __shared__ u32 badp[4];
  u64 pre = 0, tot = 0;
  u32 bad = 0;
  for (u32 j = tid; j < id.nblocks; j += 256) {
    u32 const s = blk_size[id.first_block + j];
    bad |= s == 0xFFFFFFFFu;
    u64 const v = s == 0xFFFFFFFFu ? 0u : s;
    tot += v;
    pre += j < k ? v : 0u;
  }
  for (u32 o = 32; o; o >>= 1) {
    pre += __shfl_down(pre, o, 64);
    tot += __shfl_down(tot, o, 64);
    bad |= __shfl_down(bad, o, 64);
  }
  if ((tid & 63) == 0) { part[0][tid >> 6] = pre; part[1][tid >> 6] = tot; badp[tid >> 6] = bad; }
  __syncthreads();
  pre = part[0][0] + part[0][1] + part[0][2] + part[0][3];
  tot = part[1][0] + part[1][1] + part[1][2] + part[1][3];
  bad = badp[0] | badp[1] | badp[2] | badp[3];
  bool const fail = bad || tot > id.cap;
  if (k == 0 && tid == 0) {
    item_size[d.item] = tot;
    item_status[d.item] = fail ? ZH_ST_TOO_SMALL : ZH_ST_OK;
  }
  if (fail) return;
  u32 const s = blk_size[b];
  const u8 *src = d.dst;
  u8 *dst = id.dst + pre;
  for (u32 i = tid; i < s; i += 256) dst[i] = src[i];
}

// Content checksum (reference src/cuda_zstd_manager.cu:3037-3056): one wave per
// finished frame appends the low 32 bits of XXH64 of the item's input (the first block
// already set the FHD checksum flag).
extern "C" __global__ __launch_bounds__(64) void zh_checksum_kernel(const ZhItemDesc *__restrict__ items, const ZhBlockDesc *__restrict__ descs,
                                                                   u64 *item_size, u32 *item_status) {
  u32 const it = blockIdx.x, lane = threadIdx.x;
  if (item_status[it] != ZH_ST_OK) return;
  ZhItemDesc const id = items[it];
  ZhBlockDesc const d = descs[id.first_block];
  __shared__ u64 xb[512];
  u64 const h = zh_xxh64_wave(d.src, d.frame_size, xb);
  u64 const size = item_size[it];
  __syncthreads();
  if (size + 4 > id.cap) {
    if (lane == 0) item_status[it] = ZH_ST_TOO_SMALL;
    return;
  }
  if (lane < 4) id.dst[size + lane] = (u8)(h >> (8 * lane));
  if (lane == 0) item_size[it] = size + 4;
}

namespace zh {

hipError_t init_kernels() {
  hipError_t e = lz_init();
  if (e != hipSuccess) return e;
  e = lz_deep_init();
  if (e != hipSuccess) return e;
  return entropy_init();
}

u32 lz_lds_bytes() { return zh_lz_lds_bytes(); }
u32 entropy_lds_bytes() { return zh_entropy_lds_bytes(); }

// ---- optional per-kernel event timing (bench.py roofline): events recorded on the launch stream
namespace {
struct ProfState {
  std::mutex mu;
  bool on = false;
  std::vector<hipEvent_t> pool;           // free events
  std::vector<std::vector<hipEvent_t>> pending;  // per launch: e0 (pre-K1), e1 (K1 done), e2 (K2 done), e3 (K3 done)
};
ProfState &prof() {
  static ProfState p;
  return p;
}
hipEvent_t prof_event() {
  ProfState &p = prof();
  if (!p.pool.empty()) { hipEvent_t e = p.pool.back(); p.pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
}  // namespace

void profile_enable(bool on) {
  std::lock_guard<std::mutex> g(prof().mu);
  prof().on = on;
}

// totals[0..2] = summed ms of K1, K2, K3 over the recorded launches; returns launch count
int profile_collect(double *totals) {
  ProfState &p = prof();
  std::lock_guard<std::mutex> g(p.mu);
  totals[0] = totals[1] = totals[2] = 0;
  int n = 0;
  for (auto &ev : p.pending) {
    (void)hipEventSynchronize(ev[3]);
    float a = 0, b = 0, c = 0;
    (void)hipEventElapsedTime(&a, ev[0], ev[1]);
    (void)hipEventElapsedTime(&b, ev[1], ev[2]);
    (void)hipEventElapsedTime(&c, ev[2], ev[3]);
    totals[0] += a; totals[1] += b; totals[2] += c;
    for (auto e : ev) p.pool.push_back(e);
    n++;
  }
  p.pending.clear();
  return n;
}

hipError_t launch_compress(const ZhBatch &b, hipStream_t stream) {
  if (b.nblocks == 0) return hipSuccess;
  std::vector<hipEvent_t> ev;
  {
    std::lock_guard<std::mutex> g(prof().mu);
    if (prof().on) for (int k = 0; k < 4; k++) ev.push_back(prof_event());
  }
  if (!ev.empty()) (void)hipEventRecord(ev[0], stream);
  if (b.ranges) {
    // four launches whatever the mix (the host cannot see which classes are empty): the three K1
    // parses, then the deep matcher over all its depths
    lz_launch_ranged(b.descs, b.nblocks, b.ws, b.ranges, stream);
    hipError_t const e = lz_deep_launch_ranged(b.descs, b.nblocks, b.ws, b.ranges, b.blk_level, stream);
    if (e != hipSuccess) return e;
  } else if (b.level >= ZH_DEEP_LEVEL) {
    // levels >= ZH_DEEP_LEVEL: the deep chain matcher; below: K1's dual-hash parse
    (void)hipMemsetAsync(b.ws.ctr, 0, 4, stream);  // the matcher's block counter
    hipError_t const e = lz_deep_launch(b.descs, b.nblocks, b.ws, b.level, stream);
    if (e != hipSuccess) return e;
  } else {
    (void)hipMemsetAsync(b.ws.ctr, 0, 4, stream);  // K1's block counter
    lz_launch(b.descs, b.nblocks, b.ws, (u32)ZH_K1_MODE(b.level), stream);
  }
  if (!ev.empty()) (void)hipEventRecord(ev[1], stream);
  entropy_launch(b.descs, b.nblocks, b.ws, b.window_log, b.block_size, b.item_size, b.item_status, b.blk_size, b.blk_level, stream);
  if (!ev.empty()) (void)hipEventRecord(ev[2], stream);
  if (b.gather && b.nitems)
    hipLaunchKernelGGL(zh_gather_kernel, dim3(b.nblocks), dim3(256), 0, stream, b.items, b.descs, b.blk_size, b.item_size, b.item_status);
  if (b.checksum && b.nitems)
    hipLaunchKernelGGL(zh_checksum_kernel, dim3(b.nitems), dim3(64), 0, stream, b.items, b.descs, b.item_size, b.item_status);
  if (!ev.empty()) {
    (void)hipEventRecord(ev[3], stream);
    std::lock_guard<std::mutex> g(prof().mu);
    prof().pending.push_back(ev);
  }
  return hipGetLastError();
}

hipError_t launch_plan(const ZhBatch &b, const ZhPlanArrays &a, hipStream_t stream) {
  if (!b.nblocks) return hipSuccess;
  dim3 const grid((b.nblocks + 255) / 256);
  if (a.levels) {
    if (b.nitems > ZH_RANK_MAX_ITEMS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(zh_rank_kernel, dim3(1), dim3(ZH_SCAN_THREADS), 0, stream, a.levels, b.nitems, b.nblocks / b.nitems, b.rank, b.ranges);
    hipLaunchKernelGGL(zh_plan_levels_kernel, grid, dim3(256), 0, stream, b, a);
  } else {
    hipLaunchKernelGGL(zh_plan_kernel, grid, dim3(256), 0, stream, b, a);
  }
  return hipGetLastError();
}

}  // namespace zh

// zh_host.cpp — C++17 host runtime, the batch manager: workspace layouts, dictionaries on the device,
// ZstdBatchManager, DictionarySet, the factories and the one-shot calls (the other subsystems: zh_host_*.cpp).
//
// Host side of the reference's L3/L4: ZstdBatchManager /
// NvcompV5BatchManager / HybridEngine / C API, redesigned around one batched
// device pipeline (K1 zh_lz_kernel -> K2 zh_entropy_kernel -> [K3 gather]) with a
// single host synchronisation per call instead of the reference's ~13 per block
// (src/cuda_zstd_manager.cu:2328-3112).
#include "zh_dict.h"
#include "zh_dict_entropy.h"
#include "zh_host.h"

namespace cuda_zstd {
namespace {
// Long-distance matching applies to a frame of n bytes: asked for, no dictionary or history, a
// window that reaches past one block, more than one device block, 32-bit positions
inline bool ldm_applies(const CompressionConfig &c, size_t n, bool has_dict) {
  return c.enable_ldm && !has_dict && c.window_log >= ZH_HIST_WINDOW_LOG && n > (size_t)ZH_BLOCK_MAX && n <= ZH_LDM_MAX_FRAME;
}

// What a compress call's workspace depends on.  Every size query and every compress entry builds
// its shape here, so a query and the call it sizes for cannot disagree.
struct BatchShape {
  size_t nblocks = 0, nitems = 0;
  bool staged = false;   // some frame has more than one block: staging slots, the gather
  bool deep = false;     // a level >= ZH_DEEP_LEVEL call: the deep matcher's scratch slots
  bool levels = false;   // a mixed-level batch: ranks, level bytes, class ranges
  size_t ldm_cells = 0;  // a long-distance-matching call over one frame of that many cells (three block slots each)
  u32 ldm_tlog = 0;      // with its table of 2^ldm_tlog entries
  // the host plan: frames of these sizes, one after the other
  BatchShape(const size_t *sizes, size_t count, const CompressionConfig &c, bool has_dict) : nitems(count), deep(c.level >= ZH_DEEP_LEVEL) {
    for (size_t i = 0; i < count; i++) {
      size_t const nb = zh_frame_blocks(sizes[i], zh_split_dict(c.level, has_dict));
      nblocks += nb;
      staged |= nb > 1;
    }
  }
  // the device plans: every item takes the block slots of a frame of max_chunk bytes (at least one)
  BatchShape(size_t count, size_t max_chunk, int level, bool split_dict) : nitems(count), deep(level >= ZH_DEEP_LEVEL) {
    size_t const bpi = std::max<size_t>(1, zh_frame_blocks(max_chunk, split_dict));
    nblocks = count * bpi;
    staged = bpi > 1;
  }
  // a mixed-level batch: any item may be deep; no dictionary
  static BatchShape mixed_levels(size_t count, size_t max_chunk) { BatchShape s(count, max_chunk, ZH_DEEP_LEVEL, false); s.levels = true; return s; }
  // compress() of one frame long-distance matching applies to
  static BatchShape ldm_frame(const CompressionConfig &c, size_t n) {
    BatchShape s(1, n, c.level, false);
    s.ldm_cells = s.nblocks;
    s.nblocks *= 3;
    s.staged = true;
    s.ldm_tlog = zh_ldm_table_log(n, c.ldm_hash_log);
    return s;
  }
};

// Workspace layout inside the caller's temp buffer: the regions every call has, then the deep
// matcher's scratch slots (one per persistent workgroup), then the long-distance finder's table,
// per-cell sample lists and records, then a mixed-level batch's ranks, level bytes and class ranges
// (the optional regions are empty when the shape does not ask for them)
struct WsLayout {
  size_t descs, items, blk_size, item_size, item_status, staging, counter, blocks, deep, deep_slots, total;
  size_t ldm_table, ldm_skey, ldm_sslot, ldm_scount, ldm_rec;
  size_t rank, blk_level, ranges;
  BatchShape shape;
  explicit WsLayout(const BatchShape &s) : shape(s) {
    size_t const nblocks = s.nblocks, nitems = s.nitems, cells = s.ldm_cells;
    Carve c;
    descs = c.take(nblocks * sizeof(ZhBlockDesc));
    items = c.take(nitems * sizeof(ZhItemDesc));
    blk_size = c.take(nblocks * 4);
    item_size = c.take(nitems * 8);
    item_status = c.take(nitems * 4);
    staging = c.take(s.staged ? nblocks * (size_t)ZH_STAGE_SLOT : 0);
    counter = c.take(4);
    blocks = c.take(nblocks * (size_t)ZH_WS_BLOCK_BYTES);
    deep_slots = s.deep ? std::min(nblocks, (size_t)ZH_DEEP_SLOTS_MAX) : 0;
    deep = c.take(deep_slots * ZH_DEEP_SLOT_BYTES);
    ldm_table = c.take(cells ? sizeof(u64) << s.ldm_tlog : 0);
    ldm_skey = c.take(cells * ZH_LDM_CELL_SAMPLES * sizeof(u64));
    ldm_sslot = c.take(cells * ZH_LDM_CELL_SAMPLES * sizeof(u32));
    ldm_scount = c.take(cells * sizeof(u32));
    ldm_rec = c.take(cells * sizeof(ZhLdmRecord));
    rank = c.take(s.levels ? nitems * 4 : 0);
    blk_level = c.take(s.levels ? nblocks : 0);
    ranges = c.take(s.levels ? sizeof(ZhClassRanges) : 0);
    total = c.o + 256;  // slack for base alignment
  }
};

// Decoder workspace (zh_decode.hip): per-item arrays (host-array entry points upload
// them), then one slot per item holding the literals and sequence records of the block
// being decoded.  A slot is sized for blocks of block_cap regenerated bytes: 128 KiB
// (the format's maximum) unless every output capacity is smaller.
struct DecLayout {
  size_t in_ptrs, in_sizes, out_ptrs, caps, out_sizes, statuses, slots, total;
  u32 block_cap, lit_bytes, seq_cap, ho_off;
  u64 slot_bytes;
  static constexpr size_t kBlockMax = 128 * 1024;
  static DecLayout make(size_t n, size_t max_block) {
    DecLayout L{};
    L.block_cap = (u32)std::min(std::max<size_t>(max_block, 64), kBlockMax);
    L.lit_bytes = (u32)align256(L.block_cap + 64);
    L.seq_cap = L.block_cap / 3 + 2;
    L.ho_off = (u32)(L.lit_bytes + align256((size_t)L.seq_cap * 8));
    L.slot_bytes = L.ho_off + align256(ZH_DEC_HANDOFF_BYTES);
    Carve c;
    L.in_ptrs = c.take(n * 8);
    L.in_sizes = c.take(n * 8);
    L.out_ptrs = c.take(n * 8);
    L.caps = c.take(n * 8);
    L.out_sizes = c.take(n * 8);
    L.statuses = c.take(n * 4);
    L.slots = c.take(n * L.slot_bytes);
    L.total = c.o + 256;  // slack for base alignment
    return L;
  }
  ZhDecArgs args(u8 *base) const {
    ZhDecArgs a{};
    a.ws = base + slots;
    a.slot_bytes = slot_bytes;
    a.lit_bytes = lit_bytes;
    a.block_cap = block_cap;
    a.seq_cap = seq_cap;
    a.ho_off = ho_off;
    return a;
  }
};

Status from_dec_status(u32 s) {
  switch (s) {
    case 0: return Status::SUCCESS;
    case 2: return Status::ERROR_INVALID_PARAMETER;
    case 5: return Status::ERROR_INVALID_MAGIC;
    case 6: return Status::ERROR_CORRUPT_DATA;
    case 7: return Status::ERROR_BUFFER_TOO_SMALL;
    case 9: return Status::ERROR_DICTIONARY_MISMATCH;
    case 10: return Status::ERROR_CHECKSUM_FAILED;
    default: return Status::ERROR_DECOMPRESSION;
  }
}

// Stream-ordered launches that may still read a dictionary's device memory: one event per stream,
// recorded after each launch (the blocking entry points have finished reading when they return).
// Whoever owns the memory waits for them before it frees it.
struct StreamUses {
  std::mutex mu;
  std::vector<std::pair<hipStream_t, hipEvent_t>> events;
  StreamUses() = default;
  StreamUses(const StreamUses &) = delete;
  StreamUses &operator=(const StreamUses &) = delete;
  ~StreamUses() {
    for (auto &u : events) (void)hipEventDestroy(u.second);
  }
  // a stream-ordered launch on `stream` reads the memory
  Status note(hipStream_t stream) {
    std::lock_guard<std::mutex> g(mu);
    for (auto &u : events)
      if (u.first == stream) return hipEventRecord(u.second, stream) == hipSuccess ? Status::SUCCESS : Status::ERROR_CUDA_ERROR;
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return Status::ERROR_CUDA_ERROR;
    events.emplace_back(stream, e);
    return hipEventRecord(e, stream) == hipSuccess ? Status::SUCCESS : Status::ERROR_CUDA_ERROR;
  }
  // every noted launch has finished
  Status wait() {
    std::lock_guard<std::mutex> g(mu);
    Status s = Status::SUCCESS;
    for (auto &u : events)
      if (hipEventSynchronize(u.second) != hipSuccess) s = Status::ERROR_CUDA_ERROR;
    return s;
  }
};

// A set of dictionaries on the device (zh_dictset.h): one allocation holding, per entry, the whole
// buffer (the decoder reads a formatted dictionary's tables and repcodes from it), K1's hash tables
// and the deep matcher's chains of the content tail (every record's first block starts from them
// instead of hashing the dictionary again) and a formatted dictionary's entropy blob as the entropy
// kernel reads it (zh_dict_entropy.h), indexed by an entry table, with the non-zero IDs sorted next
// to it.  Immutable once built.  The tables come from the one pair of builders (the dictionary is a
// grid dimension), ZH_DICTSET_GROUP dictionaries at a time so that the build's scratch is bounded:
// four stream operations per group, whatever the set's size.  A handle's own dictionary is a set of
// one (DevDict).
#define ZH_DICTSET_GROUP 64u
struct DictSetDev {
  u8 *mem = nullptr;
  size_t mem_bytes = 0;
  std::vector<ZhDictSetEntry> ents;  // (device pointers)
  std::vector<ZhDictSetId> ids;      // the non-zero IDs, sorted
  const ZhDictSetEntry *d_ents = nullptr;
  const ZhDictSetId *d_ids = nullptr;
  StreamUses uses;  // stream-ordered launches that may still read the set
  DictSetDev() = default;
  DictSetDev(const DictSetDev &) = delete;
  DictSetDev &operator=(const DictSetDev &) = delete;
  ~DictSetDev() {
    (void)uses.wait();
    if (mem) (void)hipFree(mem);
  }
  u32 count() const { return (u32)ents.size(); }
  int find(u32 id) const { return zh_dictset_find(ids.data(), (u32)ids.size(), id); }
  // the decoder's view; dict_index: one entry index per item (device array) or null
  void fill(ZhDecArgs &a, const int32_t *dict_index) const {
    a.set = d_ents;
    a.set_ids = d_ids;
    a.set_count = count();
    a.set_nids = (u32)ids.size();
    a.dict_index = dict_index;
  }
  // bufs[i] / sizes[i]: host bytes of dictionary i, raw content or formatted, 1 .. kDictMaxBytes of
  // them (a set's floor of MIN_DICT_SIZE is DictionarySet::create's rule).  need_tables false: a
  // build whose table stage fails leaves the (host) entries without tables and succeeds.
  Status build(const u8 *const *bufs, const size_t *sizes, size_t n, hipStream_t stream, bool need_tables = true) {
    if (!bufs || !sizes || n < 1 || n > ZH_DICTSET_MAX) return Status::ERROR_INVALID_PARAMETER;
    Status s = ensure_kernels();
    if (s != Status::SUCCESS) return s;
    std::vector<u32> raw_ids(n);
    std::vector<size_t> offs(n);
    for (size_t i = 0; i < n; i++) {
      if (!bufs[i] || !sizes[i] || sizes[i] > zh::kDictMaxBytes) return Status::ERROR_INVALID_PARAMETER;
      if (!zh::dict_layout(bufs[i], sizes[i], raw_ids[i], offs[i])) return Status::ERROR_DICTIONARY_FAILED;
    }
    ids.resize(n);
    u32 nids = 0;
    if (!zh_dictset_sort_ids(raw_ids.data(), n, ids.data(), &nids)) return Status::ERROR_INVALID_PARAMETER;  // a shared non-zero ID
    ids.resize(nids);
    // layout: the uploaded part (entry table, IDs, build jobs, buffers, entropy blobs), then the tables
    Carve c;
    size_t const o_ents = c.take(n * sizeof(ZhDictSetEntry)), o_ids = c.take(n * sizeof(ZhDictSetId)), o_jobs = c.take(n * sizeof(ZhDictBuildJob));
    std::vector<size_t> o_buf(n), o_dent(n, 0), o_dtab(n, 0), o_prev(n, 0), o_head(n, 0);
    std::vector<ZhDictEnt> blobs(n);
    std::vector<u8> has_ent(n, 0);
    for (size_t i = 0; i < n; i++) {
      o_buf[i] = c.take(sizes[i]);
      // a formatted dictionary: its Huffman code, FSE encoding tables, bit costs and repcodes
      // (none for a section the encoder cannot use)
      size_t co2 = 0;
      if (offs[i] && zh::dent::parse(bufs[i], sizes[i], &blobs[i], &co2) && co2 == offs[i]) {
        has_ent[i] = 1;
        o_dent[i] = c.take(sizeof(ZhDictEnt));
      }
    }
    size_t const upload = c.o;
    size_t const tab_entries = (size_t(1) << ZH_HASH_LOG_LONG) + (size_t(1) << ZH_HASH_LOG_SHORT);
    ents.assign(n, ZhDictSetEntry{});
    std::vector<ZhDictBuildJob> jobs(n);
    for (size_t i = 0; i < n; i++) {
      size_t const cn = sizes[i] - offs[i];
      ZhDictSetEntry &e = ents[i];
      e.n = (u32)sizes[i];
      e.off = (u32)offs[i];
      e.id = raw_ids[i];
      e.dtab_P = zh::lz_dict_tables_P(cn);
      zh::lz_deep_dict_shape(cn, e.dd_pre, e.dd_split);
      if (e.dtab_P) o_dtab[i] = c.take(tab_entries * 2);
      if (e.dd_pre) {
        o_prev[i] = c.take((size_t)e.dd_split * 4);
        o_head[i] = c.take(size_t(4) << ZH_HASH_LOG_SHORT);
      }
    }
    mem_bytes = c.o;
    if (hipMalloc(&mem, mem_bytes) != hipSuccess) { mem = nullptr; return Status::ERROR_OUT_OF_MEMORY; }
    for (size_t i = 0; i < n; i++) {
      ZhDictSetEntry &e = ents[i];
      size_t const cn = sizes[i] - offs[i];
      e.buf = mem + o_buf[i];
      e.dtab = e.dtab_P ? (const u16 *)(mem + o_dtab[i]) : nullptr;
      e.dd_prev = e.dd_pre ? (const u32 *)(mem + o_prev[i]) : nullptr;
      e.dd_head = e.dd_pre ? (const u32 *)(mem + o_head[i]) : nullptr;
      e.dent = has_ent[i] ? (const ZhDictEnt *)(mem + o_dent[i]) : nullptr;
      ZhDictBuildJob &j = jobs[i];
      j.tail = e.buf + e.off + cn - e.dtab_P;
      j.dtab = (u16 *)e.dtab;
      j.B = e.dtab_P ? e.dtab_P - ZH_DTAB_MARGIN : 0u;
      j.dtail = e.buf + e.off + cn - e.dd_pre;
      j.dprev = (u32 *)e.dd_prev;
      j.dhead = (u32 *)e.dd_head;
      j.dP = e.dd_pre;
    }
    std::vector<u8> h(upload);
    memcpy(h.data() + o_ents, ents.data(), n * sizeof(ZhDictSetEntry));
    if (nids) memcpy(h.data() + o_ids, ids.data(), nids * sizeof(ZhDictSetId));
    memcpy(h.data() + o_jobs, jobs.data(), n * sizeof(ZhDictBuildJob));
    for (size_t i = 0; i < n; i++) {
      memcpy(h.data() + o_buf[i], bufs[i], sizes[i]);
      if (has_ent[i]) memcpy(h.data() + o_dent[i], &blobs[i], sizeof(ZhDictEnt));
    }
    if (hipMemcpy(mem, h.data(), upload, hipMemcpyHostToDevice) != hipSuccess) return Status::ERROR_CUDA_ERROR;
    d_ents = (const ZhDictSetEntry *)(mem + o_ents);
    d_ids = (const ZhDictSetId *)(mem + o_ids);
    // the tables, a group at a time
    u32 const group = (u32)std::min<size_t>(n, ZH_DICTSET_GROUP);
    size_t const tmp_bytes = align256((size_t)group * tab_entries * 4);
    u8 *scratch = nullptr;
    s = hipMalloc(&scratch, tmp_bytes + (size_t)group * ZH_DEEP_DICT_STG) == hipSuccess ? Status::SUCCESS : Status::ERROR_OUT_OF_MEMORY;
    if (s == Status::SUCCESS) {
      const ZhDictBuildJob *const d_jobs = (const ZhDictBuildJob *)(mem + o_jobs);
      hipError_t e = hipSuccess;
      for (size_t g0 = 0; g0 < n && e == hipSuccess; g0 += group) {
        u32 const cnt = (u32)std::min<size_t>(group, n - g0);
        e = zh::lz_dict_tables_batch(d_jobs + g0, cnt, (u32 *)scratch, stream);
        if (e == hipSuccess) e = zh::lz_deep_dict_tables_batch(d_jobs + g0, cnt, scratch + tmp_bytes, stream);
      }
      if (hipStreamSynchronize(stream) != hipSuccess || e != hipSuccess) s = Status::ERROR_CUDA_ERROR;
      (void)hipFree(scratch);
    }
    if (s == Status::SUCCESS || need_tables) return s;
    for (ZhDictSetEntry &e : ents) {
      e.dtab = nullptr;
      e.dd_prev = e.dd_head = nullptr;
      e.dtab_P = e.dd_pre = e.dd_split = 0;
    }
    return Status::SUCCESS;
  }
};

// A handle's dictionary, or a stream's history, on the device: one entry
// (zh_dictset.h) and what owns its memory.  A loaded dictionary is the entry of a one-entry set,
// built as any set is.  A view is an entry of caller memory without tables.
struct DevDict {
  ZhDictSetEntry e{};               // n 0: none
  std::unique_ptr<DictSetDev> own;  // the set e is entry 0 of (null: a view, or nothing loaded)
  std::vector<u8> host;             // the loaded bytes (a reload of the same dictionary keeps everything)
  // raw-content view of device-resident history (never freed here; a moving window: hashed by
  // every block).  (An entry's size has 32 bits: the bytes next to the data, and no match reaches
  // further back.)
  static void view(DevDict &v, const void *p, size_t bytes) {
    size_t const n = std::min<size_t>(bytes, 0xFFFFFFFFu);
    v.e = ZhDictSetEntry{};
    v.e.buf = (const u8 *)p + (bytes - n);
    v.e.n = (u32)n;
  }
  const u8 *content() const { return e.buf + e.off; }
  size_t content_n() const { return e.n - e.off; }
  // a stream-ordered launch on `stream` reads this dictionary
  Status note_use(hipStream_t stream) const { return own ? own->uses.note(stream) : Status::SUCCESS; }
  // raw content or a formatted dictionary (host or device buffer, 1 .. kDictMaxBytes bytes);
  // replaces the previous one, whose owner waits for the stream-ordered launches still reading it
  // before its memory goes
  Status load(const void *p, size_t bytes, hipStream_t stream) {
    if (!p || !bytes || bytes > zh::kDictMaxBytes) return Status::ERROR_INVALID_PARAMETER;
    std::vector<u8> h(bytes);
    Status s = copy_any(h.data(), p, bytes, stream);
    if (s != Status::SUCCESS) return s;
    if (own && e.n == bytes && host == h) return Status::SUCCESS;  // the same dictionary: tables kept
    auto set = std::make_unique<DictSetDev>();
    const u8 *const buf = h.data();
    s = set->build(&buf, &bytes, 1, stream, false);
    if (s != Status::SUCCESS) return s;
    own = std::move(set);
    e = own->ents[0];
    host.swap(h);
    return Status::SUCCESS;
  }
  // the blob the entropy kernel takes when the configuration asks for the dictionary's entropy section
  const ZhDictEnt *dent(const CompressionConfig &c) const { return c.dict_entropy && e.n ? e.dent : nullptr; }
  void fill(ZhDecArgs &a) const {
    if (!e.n) return;
    a.dict = e.buf;
    a.dict_n = e.n;
    a.dict_off = e.off;
    a.dict_id = e.id;
  }
};

// The batch of layout L bound to its (aligned) workspace: every pointer the plan and the stages
// take, the descriptor rule's batch constants (plan.out_cap is the caller's: one per batch on the
// device routes, one per item on the host route) and the filled ZhWorkspace.  dd: the batch's
// dictionary or null; stats: collect_entropy_stats' histograms or null.
ZhBatch bind_batch(const WsLayout &L, u8 *base, const DevDict *dd, const CompressionConfig &c, u32 *stats = nullptr) {
  if (dd && !dd->e.n) dd = nullptr;
  ZhBatch b{};
  b.descs = (ZhBlockDesc *)(base + L.descs);
  b.items = (ZhItemDesc *)(base + L.items);
  b.item_size = (u64 *)(base + L.item_size);
  b.item_status = (u32 *)(base + L.item_status);
  b.blk_size = (u32 *)(base + L.blk_size);
  b.nblocks = (u32)L.shape.nblocks;
  b.nitems = (u32)L.shape.nitems;
  b.block_size = c.block_size;
  b.level = c.level;
  b.gather = L.shape.staged;
  b.checksum = c.checksum != ChecksumPolicy::NO_COMPUTE_NO_VERIFY;
  // a mixed-level batch: every level's window reaches the previous block, and the entropy kernel
  // takes each block's window descriptor from its level byte
  b.window_log = L.shape.levels ? 0u : c.window_log;
  const ZhDictEnt *const dent = dd ? dd->dent(c) : nullptr;
  b.plan.flags = (b.checksum ? ZH_F_CHECKSUM : 0u) | (dent ? ZH_F_DICTENT : 0u) | (stats ? ZH_F_STATS : 0u);
  b.plan.hist = L.shape.levels || c.window_log >= ZH_HIST_WINDOW_LOG;
  if (dd) {
    b.plan.dict = dd->content();
    b.plan.dict_n = (u32)dd->content_n();
    b.plan.dict_id = dd->e.id;
  }
  b.plan.staging = base + L.staging;
  b.ws.base = base + L.blocks;
  b.ws.ctr = (u32 *)(base + L.counter);
  if (dd) {  // K1's tables of the dictionary's content tail and the deep matcher's chains, when the dictionary has them
    b.ws.dtab = dd->e.dtab;
    b.ws.dtab_P = dd->e.dtab_P;
    b.ws.dd_prev = dd->e.dd_prev;
    b.ws.dd_head = dd->e.dd_head;
    b.ws.dd_pre = dd->e.dd_pre;
    b.ws.dd_split = dd->e.dd_split;
  }
  b.ws.deep_slots = L.deep_slots ? base + L.deep : nullptr;
  b.ws.deep_nslots = (u32)L.deep_slots;
  b.ws.dent = dent;
  b.ws.stats = stats;
  if (L.shape.levels) {
    b.rank = (u32 *)(base + L.rank);
    b.blk_level = base + L.blk_level;
    b.ranges = (ZhClassRanges *)(base + L.ranges);
  }
  return b;
}

Status from_item_status(u32 s) {
  return s == ZH_ST_OK ? Status::SUCCESS : s == ZH_ST_TOO_SMALL ? Status::ERROR_BUFFER_TOO_SMALL : Status::ERROR_INVALID_PARAMETER;
}

// Adds the time from here to the end of the scope to one of the stats' millisecond fields
struct ScopedMs {
  double &acc;
  std::chrono::steady_clock::time_point const t0 = std::chrono::steady_clock::now();
  ~ScopedMs() { acc += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};
}  // namespace

// ============================================================================
// ZstdBatchManager
// ============================================================================
class ZstdBatchManager::Impl {
 public:
  CompressionConfig config;
  CompressionStats stats;
  dictionary::DictionaryHeader dict_hdr{};  // set_dictionary's header (dictionary_id: the frames' RFC ID)
  std::mutex api_mutex;  // one manager serialises calls (reference src/cuda_zstd_manager.cu:1542)
  void *pinned = nullptr;
  size_t pinned_bytes = 0;
  DevDict mgr_dict, call_dict;  // set_dictionary()'s / compress()'s per-call dictionary
  const DevDict *active() const { return mgr_dict.e.n ? &mgr_dict : nullptr; }
  std::shared_ptr<DictSetDev> set;  // set_dictionary_set()'s dictionary set (never together with mgr_dict)

  explicit Impl(const CompressionConfig &c) : config(c) {}
  ~Impl() { if (pinned) (void)hipHostFree(pinned); }

  void *host_scratch(size_t bytes) {
    if (bytes > pinned_bytes) {
      if (pinned) (void)hipHostFree(pinned);
      pinned = nullptr;
      pinned_bytes = 0;
      if (hipHostMalloc(&pinned, bytes, hipHostMallocDefault) != hipSuccess) { pinned = nullptr; return nullptr; }
      pinned_bytes = bytes;
    }
    return pinned;
  }

  // Who still reads the dictionary: a stream-ordered launch on `stream` read the set ds, or else
  // the manager's dictionary if one is set
  ZH_INTERNAL Status note_dict_use(const std::shared_ptr<DictSetDev> &ds, hipStream_t stream) const {
    if (ds) return ds->uses.note(stream);
    const DevDict *const dd = active();
    return dd ? dd->note_use(stream) : Status::SUCCESS;
  }

  // compress_batch_device's shape, for the manager's level and dictionary as set now
  BatchShape device_shape(size_t count, size_t max_chunk) const {
    return BatchShape(count, max_chunk, config.level, zh_split_dict(config.level, active() != nullptr));
  }

  // compress_batch_device_prefix's shape: that of a manager with a dictionary at this level
  BatchShape prefix_shape(size_t count, size_t max_chunk) const { return BatchShape(count, max_chunk, config.level, zh_split_dict(config.level, true)); }

  // The long-distance finder over one frame (layout L of BatchShape::ldm_frame): descriptors, one-sequence
  // blocks, staged sizes and records of all its cells
  hipError_t launch_ldm(const WsLayout &L, u8 *base, const void *src, size_t n, size_t cells, u32 flags, hipStream_t stream) {
    return zh::ldm_launch((const u8 *)src, n, (u32)cells, zh_ldm_table_log(n, config.ldm_hash_log), zh_ldm_max_dist(config.window_log), flags,
                          (u64 *)(base + L.ldm_table), (u64 *)(base + L.ldm_skey), (u32 *)(base + L.ldm_sslot), (u32 *)(base + L.ldm_scount),
                          (ZhBlockDesc *)(base + L.descs), base + L.staging, (u32 *)(base + L.blk_size), (ZhLdmRecord *)(base + L.ldm_rec),
                          stream);
  }

  // The device-planned entries: plan and stages, stream-ordered, nothing synchronised.  Sizes land
  // in d_out_sizes, statuses in d_statuses (or the workspace); every item's capacity is the bound of
  // max_chunk.  levels: one level per item in a.levels, read on the device -- the rank kernel sorts
  // the items by parse class, the plan writes the descriptors at their sorted slots, and the matchers
  // run over class ranges they read from the workspace; the manager's level is not used.
  // a.prefix_sizes: one prefix per item, read on the device by the plan -- an item with one gets a
  // dictionary frame's descriptors, the others plain ones, in a batch shaped like a dictionary
  // handle's (prefix_shape); ws.dtab and ws.dd_* stay null as for a view, so every first block
  // hashes its own prefix.
  // a.dict_index: one entry of the bound dictionary set per item, read on the device by the plan --
  // the entry's content is the item's prefix, its ID the frames' Dictionary_ID (zh_dictset_plan_item),
  // in the same shape; the stages take each first block's precomputed tables and entropy blob from
  // its item's entry (ws.set / ws.item_ent).
  Status run_device(const ZhPlanArrays &a, bool levels, size_t max_chunk, size_t count, size_t *d_out_sizes, int *d_statuses, void *temp,
                    size_t temp_size, hipStream_t stream) {
    // one manager serialises calls (the dictionary's use events: set_dictionary waits on them)
    std::lock_guard<std::mutex> lock(api_mutex);
    Status s = ensure_kernels();
    if (s != Status::SUCCESS) return s;
    if (!count) return Status::SUCCESS;
    if (!a.in_ptrs || !a.in_sizes || !a.out_ptrs || !d_out_sizes || max_chunk == 0) return Status::ERROR_INVALID_PARAMETER;
    // (with a dictionary set, chunks over 32 KiB take two history blocks: a larger workspace
    // than get_batch_device_temp_size's, from nvcomp_zstd_batch_get_compress_temp_size_v5)
    const DevDict *dd = active();
    // a dictionary frame's block split depends on its level (zh_split_dict): no one bpi per mixed-level batch
    if (levels && (!a.levels || dd)) return Status::ERROR_INVALID_PARAMETER;
    // one prefix source per item: not a batch dictionary too, and one level per batch
    bool const prefix = a.prefix_ptrs || a.prefix_sizes;
    if (prefix && (!a.prefix_ptrs || !a.prefix_sizes || dd || levels)) return Status::ERROR_INVALID_PARAMETER;
    // one entry of the bound set per item: one level per batch, no prefix, no long-distance matching
    std::shared_ptr<DictSetDev> const ds = a.dict_index ? set : nullptr;
    if (a.dict_index && (!ds || dd || levels || prefix || config.enable_ldm)) return Status::ERROR_INVALID_PARAMETER;
    BatchShape const shape = levels ? BatchShape::mixed_levels(count, max_chunk) : (prefix || ds) ? prefix_shape(count, max_chunk) : device_shape(count, max_chunk);
    if (levels && (count > ZH_RANK_MAX_ITEMS || shape.nblocks > 0xFFFFFFFFull)) return Status::ERROR_INVALID_PARAMETER;
    WsLayout const L(shape);
    if (!temp || temp_size < L.total) return Status::ERROR_BUFFER_TOO_SMALL;
    ZhBatch b = bind_batch(L, aligned_base(temp), dd, config);
    b.plan.out_cap = estimate_compressed_size(max_chunk, config.level);
    b.item_size = (u64 *)d_out_sizes;
    if (d_statuses) b.item_status = (u32 *)d_statuses;
    ZhPlanArrays pa = a;
    if (ds) {
      pa.set = b.ws.set = ds->d_ents;
      pa.set_count = ds->count();
      pa.set_entropy = config.dict_entropy ? 1u : 0u;
      b.ws.item_ent = a.dict_index;
    }
    hipError_t e = zh::launch_plan(b, pa, stream);
    if (e == hipSuccess) e = zh::launch_compress(b, stream);
    if (e != hipSuccess) return Status::ERROR_CUDA_ERROR;
    return note_dict_use(ds, stream);
  }

  // The device-array decoding entries (defined with them below): prefixes, or the bound dictionary
  // set with an optional entry index per buffer
  Status run_device_decompress(const void *const *d_in_ptrs, const size_t *d_in_sizes, const void *const *d_prefix_ptrs,
                               const size_t *d_prefix_sizes, const int32_t *d_dict_index, const size_t *d_out_caps, size_t max_out, size_t count,
                               void *const *d_out_ptrs, size_t *d_out_sizes, int *d_statuses, void *temp, size_t temp_size, hipStream_t stream);

  // Run the device pipeline over a list of frames given as host arrays.
  // out_sizes: in = capacity, out = bytes; statuses out.  stats_dev: collect_entropy_stats asks the
  // entropy kernel for its histograms (ZH_F_STATS).
  Status run(const void *const *in_ptrs, const size_t *in_sizes, size_t count, void *const *out_ptrs, size_t *out_sizes, Status *statuses,
             void *temp, size_t temp_size, hipStream_t stream, const DevDict *dd = nullptr, bool allow_ldm = false, u32 *stats_dev = nullptr) {
    Status s = ensure_kernels();
    if (s != Status::SUCCESS) return s;
    bool const has_dict = dd && dd->e.n;
    // long-distance matching (allow_ldm: compress() of one frame, whose workspace query sized for
    // it; the batch entries never ask): three slots per cell, the cells' descriptors come from
    // zh_ldm_cell_kernel instead of the loop below
    bool const ldm = allow_ldm && count == 1 && ldm_applies(config, in_sizes[0], has_dict);
    WsLayout const L(ldm ? BatchShape::ldm_frame(config, in_sizes[0]) : BatchShape(in_sizes, count, config, has_dict));
    size_t const nblocks = L.shape.nblocks, ldm_cells = L.shape.ldm_cells;
    if (!temp || temp_size < L.total) return Status::ERROR_BUFFER_TOO_SMALL;
    u8 *base = aligned_base(temp);
    ZhBatch batch = bind_batch(L, base, dd, config, stats_dev);

    // host plan -> one pinned upload
    size_t const up_bytes = L.blk_size;  // descs + items
    u8 *h = (u8 *)host_scratch(up_bytes + count * 12);
    if (!h) return Status::ERROR_OUT_OF_MEMORY;
    ZhBlockDesc *hd = (ZhBlockDesc *)(h + L.descs);
    ZhItemDesc *hi = (ZhItemDesc *)(h + L.items);
    u32 b = 0;
    for (size_t i = 0; i < count; i++) {
      ZhPlanItem const it{(const u8 *)in_ptrs[i], in_sizes[i], (u32)i, config.level, (u8 *)out_ptrs[i]};
      batch.plan.out_cap = out_sizes[i];
      bool invalid;  // (an empty item never gets here: the entries reject it)
      hi[i] = zh_item_desc(batch.plan, it, b, &invalid);
      if (ldm) hi[i].nblocks = (u32)nblocks;  // every slot of every cell; the finder writes the block descriptors
      else for (u32 k = 0; k < hi[i].nblocks; k++, b++) hd[b] = zh_block_desc(batch.plan, it, k, b);
    }
    if (ldm) {  // the item descriptor only; the finder's launch is stream-ordered in front of K1
      u32 const flags = batch.plan.flags | (config.level >= ZH_DEEP_LEVEL ? ZH_F_DEEP : 0u);
      if (hipMemcpyAsync(base + L.items, h + L.items, up_bytes - L.items, hipMemcpyHostToDevice, stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
      if (launch_ldm(L, base, in_ptrs[0], in_sizes[0], ldm_cells, flags, stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
    } else if (hipMemcpyAsync(base, h, up_bytes, hipMemcpyHostToDevice, stream) != hipSuccess) {
      return Status::ERROR_CUDA_ERROR;
    }
    hipError_t e = zh::launch_compress(batch, stream);
    if (e != hipSuccess) return Status::ERROR_CUDA_ERROR;
    u64 *h_size = (u64 *)(h + up_bytes);
    u32 *h_status = (u32 *)(h_size + count);
    if (hipMemcpyAsync(h_size, base + L.item_size, count * 8, hipMemcpyDeviceToHost, stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
    if (hipMemcpyAsync(h_status, base + L.item_status, count * 4, hipMemcpyDeviceToHost, stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
    if (hipStreamSynchronize(stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
    bool all_ok = true;
    for (size_t i = 0; i < count; i++) {
      Status st = from_item_status(h_status[i]);
      statuses[i] = st;
      if (st == Status::SUCCESS) out_sizes[i] = (size_t)h_size[i];
      else all_ok = false;
      stats.input_bytes += in_sizes[i];
      if (st == Status::SUCCESS) stats.output_bytes += h_size[i];
    }
    stats.blocks_processed += ldm ? ldm_cells : nblocks;  // (cells: how many of the three slots a cell fills stays on the device)
    stats.num_blocks += ldm ? ldm_cells : nblocks;
    return all_ok ? Status::SUCCESS : Status::ERROR_GENERIC;
  }

  // compress_batch() and decompress_batch(): the items with valid arguments gathered into arrays, one device call for
  // them, sizes and statuses scattered back (a failed item keeps its output_size).  The reference's compress loop
  // calls compress() per item (src/cuda_zstd_manager.cu:5744-5768), so an item below cpu_threshold takes
  // compress()'s libzstd route (without a dictionary, as compress() decides) and the rest share one device launch.
  ZH_INTERNAL Status run_items(const std::vector<BatchItem> &items, bool comp, void *temp, size_t temp_size, hipStream_t stream) {
    auto &mut = const_cast<std::vector<BatchItem> &>(items);  // the reference writes sizes/status through const (:5745)
    auto t0 = std::chrono::steady_clock::now();  // compress: the libzstd items' time counts
    const DevDict *const dd = active();
    std::vector<const void *> ip;
    std::vector<void *> op;
    std::vector<size_t> isz, osz, idx;
    bool any_bad = false;
    for (size_t i = 0; i < mut.size(); i++) {
      BatchItem &it = mut[i];
      if (!it.input_ptr || !it.output_ptr || it.input_size < (comp ? 1u : 4u)) {
        it.status = Status::ERROR_INVALID_PARAMETER;
        any_bad = true;
        continue;
      }
      if (comp && !dd && select_execution_path(it.input_size, (int)config.cpu_threshold) == ExecutionPath::CPU) {
        size_t o = it.output_size;
        it.status = cpu_compress(it.input_ptr, it.input_size, it.output_ptr, &o, config.level, stream);
        if (it.status == Status::SUCCESS) {
          it.output_size = o;
          stats.input_bytes += it.input_size;
          stats.output_bytes += o;
        } else {
          any_bad = true;
        }
        continue;
      }
      ip.push_back(it.input_ptr);
      op.push_back(it.output_ptr);
      isz.push_back(it.input_size);
      osz.push_back(it.output_size);
      idx.push_back(i);
    }
    if (!comp) {  // decode: the device call's time alone, none when no item reaches it
      if (idx.empty()) return Status::ERROR_GENERIC;
      t0 = std::chrono::steady_clock::now();
    }
    std::vector<Status> st(idx.size());
    Status const r = idx.empty() ? Status::SUCCESS
                     : comp      ? run(ip.data(), isz.data(), idx.size(), op.data(), osz.data(), st.data(), temp, temp_size, stream, dd)
                                 : run_decompress(ip.data(), isz.data(), idx.size(), op.data(), osz.data(), st.data(), temp, temp_size, stream);
    (comp ? stats.compression_time_ms : stats.decompression_time_ms) += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (r != Status::SUCCESS && r != Status::ERROR_GENERIC) return r;
    for (size_t j = 0; j < idx.size(); j++) {
      mut[idx[j]].status = st[j];
      if (st[j] == Status::SUCCESS) mut[idx[j]].output_size = osz[j];
      else any_bad = true;
    }
    return any_bad ? Status::ERROR_GENERIC : Status::SUCCESS;
  }

  // compress() and compress_with_history(): one frame through run(); a failed item's status is the call's
  ZH_INTERNAL Status compress_one(const void *in, size_t n, void *out, size_t *out_size, void *temp, size_t temp_size, hipStream_t stream,
                                  const DevDict *dd) {
    Status item;
    Status const st = run(&in, &n, 1, &out, out_size, &item, temp, temp_size, stream, dd, true);
    return st == Status::ERROR_GENERIC ? item : st;
  }

  // Decode a list of buffers given as host arrays of device pointers (one launch of
  // zh_decode_kernel, one host synchronisation).  out_sizes: in = capacity, out = bytes.
  Status run_decompress(const void *const *in_ptrs, const size_t *in_sizes, size_t count, void *const *out_ptrs, size_t *out_sizes,
                        Status *statuses, void *temp, size_t temp_size, hipStream_t stream) {
    Status s = ensure_kernels();
    if (s != Status::SUCCESS) return s;
    size_t maxcap = 0;
    for (size_t i = 0; i < count; i++) maxcap = std::max(maxcap, out_sizes[i]);
    DecLayout L = DecLayout::make(count, maxcap);
    if (!temp || temp_size < L.total) return Status::ERROR_BUFFER_TOO_SMALL;
    u8 *base = aligned_base(temp);
    size_t const up = L.out_sizes, down = L.slots - L.out_sizes;
    u8 *h = (u8 *)host_scratch(up + down);
    if (!h) return Status::ERROR_OUT_OF_MEMORY;
    for (size_t i = 0; i < count; i++) {
      ((const void **)(h + L.in_ptrs))[i] = in_ptrs[i];
      ((size_t *)(h + L.in_sizes))[i] = in_sizes[i];
      ((void **)(h + L.out_ptrs))[i] = out_ptrs[i];
      ((size_t *)(h + L.caps))[i] = out_sizes[i];
    }
    if (hipMemcpyAsync(base, h, up, hipMemcpyHostToDevice, stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
    ZhDecArgs a = L.args(base);
    mgr_dict.fill(a);
    a.in_ptrs = (const void *const *)(base + L.in_ptrs);
    a.in_sizes = (const size_t *)(base + L.in_sizes);
    a.out_ptrs = (void *const *)(base + L.out_ptrs);
    a.out_caps = (const size_t *)(base + L.caps);
    a.out_sizes = (size_t *)(base + L.out_sizes);
    a.statuses = (u32 *)(base + L.statuses);
    if (zh::launch_decompress(a, (u32)count, stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
    if (hipMemcpyAsync(h + up, base + L.out_sizes, down, hipMemcpyDeviceToHost, stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
    if (hipStreamSynchronize(stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
    const size_t *hsz = (const size_t *)(h + up);
    const u32 *hst = (const u32 *)(h + up + (L.statuses - L.out_sizes));
    bool all_ok = true;
    for (size_t i = 0; i < count; i++) {
      Status st = from_dec_status(hst[i]);
      statuses[i] = st;
      if (st == Status::SUCCESS) {
        out_sizes[i] = hsz[i];
        stats.bytes_decompressed += hsz[i];
      } else {
        all_ok = false;
      }
    }
    return all_ok ? Status::SUCCESS : Status::ERROR_GENERIC;
  }

  // One buffer, no pointer-array upload (ZhDecArgs single-item fields).  Synchronous
  // unless d_actual is given (then the size lands there, stream-ordered, 0 on error).
  Status run_decompress_one(const void *in, size_t n, void *out, size_t cap, size_t *h_actual, size_t *d_actual, void *temp, size_t temp_size,
                            hipStream_t stream, const DevDict *dd = nullptr) {
    Status s = ensure_kernels();
    if (s != Status::SUCCESS) return s;
    DecLayout L = DecLayout::make(1, cap);
    if (!temp || temp_size < L.total) return Status::ERROR_BUFFER_TOO_SMALL;
    u8 *base = aligned_base(temp);
    ZhDecArgs a = L.args(base);
    (dd ? *dd : mgr_dict).fill(a);
    a.one_in = in;
    a.one_in_size = n;
    a.one_out = out;
    a.out_cap_all = cap;
    a.out_sizes = d_actual ? d_actual : (size_t *)(base + L.out_sizes);
    a.statuses = (u32 *)(base + L.statuses);
    if (zh::launch_decompress(a, 1, stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
    if (d_actual) return Status::SUCCESS;
    u8 *h = (u8 *)host_scratch(16);
    if (!h) return Status::ERROR_OUT_OF_MEMORY;
    if (hipMemcpyAsync(h, base + L.out_sizes, 8, hipMemcpyDeviceToHost, stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
    if (hipMemcpyAsync(h + 8, base + L.statuses, 4, hipMemcpyDeviceToHost, stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
    if (hipStreamSynchronize(stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
    Status st = from_dec_status(*(const u32 *)(h + 8));
    if (st == Status::SUCCESS) {
      *h_actual = *(const size_t *)h;
      stats.bytes_decompressed += *h_actual;
    }
    return st;
  }
};

ZstdBatchManager::ZstdBatchManager() : pimpl_(new Impl(CompressionConfig::from_level(3))) {}
ZstdBatchManager::ZstdBatchManager(const CompressionConfig &c) : pimpl_(new Impl(c)) {}
ZstdBatchManager::~ZstdBatchManager() = default;

Status ZstdBatchManager::configure(const CompressionConfig &c) {
  Status s = c.validate();
  if (s != Status::SUCCESS) return s;
  pimpl_->config = c;
  return Status::SUCCESS;
}
CompressionConfig ZstdBatchManager::get_config() const { return pimpl_->config; }

// sized for the dictionary layout as well (a per-call dictionary is only known at compress())
size_t ZstdBatchManager::get_compress_temp_size(size_t n) const {
  size_t const plain = WsLayout(BatchShape(1, n, pimpl_->config.level, true)).total;
  // long-distance matching: three slots per cell, the table and the sample lists (a dictionary
  // given at compress() switches it off: the plain layout must fit too)
  return ldm_applies(pimpl_->config, n, false) ? std::max(plain, WsLayout(BatchShape::ldm_frame(pimpl_->config, n)).total) : plain;
}

Status ZstdBatchManager::collect_entropy_stats(const void *const *d_ptrs, const size_t *sizes, size_t count, unsigned int *counts,
                                               hipStream_t stream) {
  std::lock_guard<std::mutex> lock(pimpl_->api_mutex);
  if (!d_ptrs || !sizes || !counts || count == 0) return Status::ERROR_INVALID_PARAMETER;
  std::vector<size_t> isz(sizes, sizes + count), osz(count), off(count + 1, 0);
  for (size_t i = 0; i < count; i++) {
    if (!d_ptrs[i] || sizes[i] == 0) return Status::ERROR_INVALID_PARAMETER;
    osz[i] = estimate_compressed_size(sizes[i], pimpl_->config.level);
    off[i + 1] = off[i] + ((osz[i] + 255) & ~(size_t)255);
  }
  size_t const temp_bytes = WsLayout(BatchShape(isz.data(), count, pimpl_->config, pimpl_->active() != nullptr)).total;
  u8 *buf = nullptr;
  size_t const stats_off = (off[count] + 255) & ~(size_t)255, temp_off = stats_off + 4096;
  if (hipMalloc(&buf, temp_off + temp_bytes) != hipSuccess) return Status::ERROR_OUT_OF_MEMORY;
  Status s = hipMemsetAsync(buf + stats_off, 0, ZH_STATS_WORDS * sizeof(u32), stream) == hipSuccess ? Status::SUCCESS : Status::ERROR_CUDA_ERROR;
  if (s == Status::SUCCESS) {
    std::vector<void *> op(count);
    for (size_t i = 0; i < count; i++) op[i] = buf + off[i];
    std::vector<Status> st(count);
    s = pimpl_->run(d_ptrs, isz.data(), count, op.data(), osz.data(), st.data(), buf + temp_off, temp_bytes, stream, pimpl_->active(), false,
                    (u32 *)(buf + stats_off));
  }
  if (s == Status::SUCCESS && hipMemcpy(counts, buf + stats_off, ZH_STATS_WORDS * sizeof(u32), hipMemcpyDeviceToHost) != hipSuccess)
    s = Status::ERROR_CUDA_ERROR;
  (void)hipFree(buf);
  return s;
}

Status ZstdBatchManager::ldm_plan(const void *d_src, size_t size, unsigned int *host_records, size_t capacity, size_t *num_records, void *temp,
                                  size_t temp_size, hipStream_t stream) {
  std::lock_guard<std::mutex> lock(pimpl_->api_mutex);
  if (!d_src || !num_records || (capacity && !host_records) || !temp) return Status::ERROR_INVALID_PARAMETER;
  *num_records = 0;
  if (!ldm_applies(pimpl_->config, size, pimpl_->active() != nullptr)) return Status::SUCCESS;
  if (!is_device_ptr(d_src)) return Status::ERROR_INVALID_PARAMETER;
  Status s = ensure_kernels();
  if (s != Status::SUCCESS) return s;
  WsLayout const L(BatchShape::ldm_frame(pimpl_->config, size));
  size_t const cells = L.shape.ldm_cells;
  if (temp_size < L.total) return Status::ERROR_BUFFER_TOO_SMALL;
  if (capacity < cells) return Status::ERROR_BUFFER_TOO_SMALL;
  u8 *base = aligned_base(temp);
  if (pimpl_->launch_ldm(L, base, d_src, size, cells, 0, stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
  if (hipMemcpyAsync(host_records, base + L.ldm_rec, cells * sizeof(ZhLdmRecord), hipMemcpyDeviceToHost, stream) != hipSuccess)
    return Status::ERROR_CUDA_ERROR;
  if (hipStreamSynchronize(stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
  *num_records = cells;
  return Status::SUCCESS;
}
// one slot for 128 KiB blocks (reference src/cuda_zstd_manager.cu:1373-1408 also sizes for one block)
size_t ZstdBatchManager::get_decompress_temp_size(size_t) const { return DecLayout::make(1, DecLayout::kBlockMax).total; }
size_t ZstdBatchManager::get_max_compressed_size(size_t n) const { return estimate_compressed_size(n, pimpl_->config.level); }

Status ZstdBatchManager::compress(const void *in, size_t n, void *out, size_t *out_size, void *temp, size_t temp_size, const void *dict_buffer,
                                  size_t dict_size, hipStream_t stream, void *) {
  std::lock_guard<std::mutex> lock(pimpl_->api_mutex);
  // reference validation order (src/cuda_zstd_manager.cu:1549-1565)
  if (!in || !out || !out_size || !temp) return Status::ERROR_INVALID_PARAMETER;
  if (n == 0) { *out_size = 0; return Status::ERROR_INVALID_PARAMETER; }
  if (temp_size < get_compress_temp_size(n)) return Status::ERROR_BUFFER_TOO_SMALL;
  // a per-call dictionary (host or device buffer) overrides the manager's set_dictionary()
  const DevDict *dd = pimpl_->active();
  if (dict_buffer && dict_size) {
    Status s = pimpl_->call_dict.load(dict_buffer, dict_size, stream);
    if (s != Status::SUCCESS) return s;
    dd = &pimpl_->call_dict;
  }
  ScopedMs const timed{pimpl_->stats.compression_time_ms};
  if (dd || select_execution_path(n, (int)pimpl_->config.cpu_threshold) != ExecutionPath::CPU)
    return pimpl_->compress_one(in, n, out, out_size, temp, temp_size, stream, dd);
  Status const st = cpu_compress(in, n, out, out_size, pimpl_->config.level, stream);
  if (st == Status::SUCCESS) { pimpl_->stats.input_bytes += n; pimpl_->stats.output_bytes += *out_size; }
  return st;
}

// GPU decode (zh_decode.hip) of device-resident frames; validation order of the
// reference (src/cuda_zstd_manager.cu:3203-3212).  *out_size: capacity in, bytes out.
Status ZstdBatchManager::decompress(const void *in, size_t n, void *out, size_t *out_size, void *temp, size_t temp_size, hipStream_t stream) {
  std::lock_guard<std::mutex> lock(pimpl_->api_mutex);
  if (!in || !out || !out_size || !temp || n < 4) return Status::ERROR_INVALID_PARAMETER;
  // the slot the decode actually uses: sized by the output capacity, so a workspace from
  // allocate_inference_workspace(max_out) is enough (reference tests/test_inference_api.cu:398-410)
  if (temp_size < DecLayout::make(1, *out_size).total) return Status::ERROR_BUFFER_TOO_SMALL;
  if (!is_device_ptr(in) || !is_device_ptr(out)) return Status::ERROR_INVALID_PARAMETER;  // device-resident API
  ScopedMs const timed{pimpl_->stats.decompression_time_ms};
  return pimpl_->run_decompress_one(in, n, out, *out_size, out_size, nullptr, temp, temp_size, stream);  // (*out_size: written on success only)
}

Status ZstdBatchManager::compress_with_history(const void *in, size_t n, void *out, size_t *out_size, void *temp, size_t temp_size,
                                               const void *hist, size_t hist_n, hipStream_t stream) {
  std::lock_guard<std::mutex> lock(pimpl_->api_mutex);
  if (!in || !out || !out_size || !temp || (hist_n && !hist)) return Status::ERROR_INVALID_PARAMETER;
  if (n == 0) { *out_size = 0; return Status::ERROR_INVALID_PARAMETER; }
  if (temp_size < get_compress_temp_size(n)) return Status::ERROR_BUFFER_TOO_SMALL;
  DevDict view;
  if (hist_n) DevDict::view(view, hist, hist_n);
  ScopedMs const timed{pimpl_->stats.compression_time_ms};
  return pimpl_->compress_one(in, n, out, out_size, temp, temp_size, stream, hist_n ? &view : pimpl_->active());
}
Status ZstdBatchManager::decompress_with_history(const void *in, size_t n, void *out, size_t *out_size, void *temp, size_t temp_size,
                                                 const void *hist, size_t hist_n, hipStream_t stream) {
  std::lock_guard<std::mutex> lock(pimpl_->api_mutex);
  if (!in || !out || !out_size || !temp || n < 4 || (hist_n && !hist)) return Status::ERROR_INVALID_PARAMETER;
  if (temp_size < DecLayout::make(1, *out_size).total) return Status::ERROR_BUFFER_TOO_SMALL;
  DevDict view;
  if (hist_n) DevDict::view(view, hist, hist_n);
  return pimpl_->run_decompress_one(in, n, out, *out_size, out_size, nullptr, temp, temp_size, stream, hist_n ? &view : nullptr);
}

// Dictionary compression and decompression: raw content or a formatted RFC 8878
// dictionary; copied to the device once (the reference keeps a shallow pointer and copies it
// into the workspace per call, src/cuda_zstd_manager.cu:1699-1775, 3711-3764)
// The reference's checks (src/cuda_zstd_manager.cu:3711-3736): content present, MIN_DICT_SIZE ..
// MAX_DICT_SIZE bytes.  raw_content may be host or device memory (copied once, DevDict::load).
Status ZstdBatchManager::set_dictionary(const dictionary::Dictionary &d) {
  std::lock_guard<std::mutex> lock(pimpl_->api_mutex);
  if (!d.raw_content || d.raw_size == 0) return Status::ERROR_INVALID_PARAMETER;
  if (d.raw_size < dictionary::MIN_DICT_SIZE || d.raw_size > dictionary::MAX_DICT_SIZE) return Status::ERROR_INVALID_PARAMETER;
  if (pimpl_->set) return Status::ERROR_INVALID_PARAMETER;  // a dictionary set is bound: one or the other
  Status s = pimpl_->mgr_dict.load(d.raw_content, d.raw_size, 0);
  if (s != Status::SUCCESS) return s;
  pimpl_->dict_hdr = d.header;
  pimpl_->dict_hdr.dictionary_id = pimpl_->mgr_dict.e.id;
  pimpl_->dict_hdr.raw_content_size = d.raw_size;
  return Status::SUCCESS;
}
// reference :3858-3863: no dictionary -> ERROR_INVALID_PARAMETER; else a deep copy (the caller
// frees dict.raw_content with free(), Dictionary's copy semantics)
Status ZstdBatchManager::get_dictionary(dictionary::Dictionary &d) const {
  std::lock_guard<std::mutex> lock(pimpl_->api_mutex);  // set_dictionary swaps mgr_dict under it
  if (!pimpl_->active()) return Status::ERROR_INVALID_PARAMETER;
  dictionary::Dictionary view;
  view.header = pimpl_->dict_hdr;
  view.raw_content = pimpl_->mgr_dict.host.data();
  view.raw_size = (u32)pimpl_->mgr_dict.host.size();
  d = view;
  return d.raw_content ? Status::SUCCESS : Status::ERROR_OUT_OF_MEMORY;
}
Status ZstdBatchManager::clear_dictionary() {
  std::lock_guard<std::mutex> lock(pimpl_->api_mutex);
  pimpl_->dict_hdr = dictionary::DictionaryHeader{};
  pimpl_->mgr_dict.e.n = 0;
  return Status::SUCCESS;
}
const CompressionStats &ZstdBatchManager::get_stats() const { return pimpl_->stats; }
Status ZstdBatchManager::set_compression_level(int level) {
  if (!is_valid_compression_level(level)) return Status::ERROR_INVALID_PARAMETER;
  CompressionConfig c = pimpl_->config;
  c.level = level;
  apply_level_parameters(c);
  pimpl_->config = c;
  return Status::SUCCESS;
}
int ZstdBatchManager::get_compression_level() const { return pimpl_->config.level; }
void ZstdBatchManager::reset_stats() { pimpl_->stats = CompressionStats{}; }

size_t ZstdBatchManager::get_batch_compress_temp_size(const std::vector<size_t> &sizes) const {
  // (for the manager's dictionary as set now -- compress_batch takes no per-call dictionary; a
  // dictionary set later may need more: ZH_FRAME_BLOCK, and the call then fails with
  // ERROR_BUFFER_TOO_SMALL)
  return WsLayout(BatchShape(sizes.data(), sizes.size(), pimpl_->config, pimpl_->active() != nullptr)).total;
}
size_t ZstdBatchManager::get_batch_decompress_temp_size(const std::vector<size_t> &sizes) const {
  return DecLayout::make(std::max<size_t>(1, sizes.size()), DecLayout::kBlockMax).total;
}

Status ZstdBatchManager::compress_batch(const std::vector<BatchItem> &items, void *temp, size_t temp_size, hipStream_t stream) {
  std::lock_guard<std::mutex> lock(pimpl_->api_mutex);
  reset_stats();
  if (items.empty()) return Status::SUCCESS;
  std::vector<size_t> sizes(items.size());
  for (size_t i = 0; i < items.size(); i++) sizes[i] = items[i].input_size;
  if (temp_size < get_batch_compress_temp_size(sizes)) return Status::ERROR_BUFFER_TOO_SMALL;
  return pimpl_->run_items(items, true, temp, temp_size, stream);
}

// ZstdBatchManager::decompress_batch (reference src/cuda_zstd_manager.cu:5799-5885): every
// item decoded by one launch; output_size in = capacity, out = bytes; per-item status.
Status ZstdBatchManager::decompress_batch(const std::vector<BatchItem> &items, void *temp, size_t temp_size, hipStream_t stream) {
  std::lock_guard<std::mutex> lock(pimpl_->api_mutex);
  if (items.empty()) return Status::SUCCESS;
  return pimpl_->run_items(items, false, temp, temp_size, stream);
}

Status ZstdBatchManager::decompress_to_preallocated(const void *in, size_t n, void *out, size_t cap, size_t *actual, void *temp, size_t temp_size,
                                                    hipStream_t stream) {
  if (!in || !out || !actual) return Status::ERROR_INVALID_PARAMETER;
  if (cap == 0) return Status::ERROR_BUFFER_TOO_SMALL;  // reference tests/test_inference_api.cu:581-586
  *actual = cap;
  return decompress(in, n, out, actual, temp, temp_size, stream);
}
Status ZstdBatchManager::decompress_batch_preallocated(std::vector<BatchItem> &items, void *t, size_t ts, hipStream_t stream) {
  return decompress_batch(items, t, ts, stream);
}
// stream-ordered: nothing is synchronised; *d_actual (device) receives the size, 0 on error
Status ZstdBatchManager::decompress_async_no_sync(const void *in, size_t n, void *out, size_t cap, size_t *d_actual, void *temp, size_t temp_size,
                                                  hipStream_t stream) {
  std::lock_guard<std::mutex> lock(pimpl_->api_mutex);
  if (!in || !out || !d_actual || !temp || n < 4) return Status::ERROR_INVALID_PARAMETER;
  if (temp_size < DecLayout::make(1, cap).total) return Status::ERROR_BUFFER_TOO_SMALL;
  return pimpl_->run_decompress_one(in, n, out, cap, nullptr, d_actual, temp, temp_size, stream);
}
size_t ZstdBatchManager::get_inference_workspace_size(size_t, size_t max_out) const { return DecLayout::make(1, max_out).total; }
Status ZstdBatchManager::allocate_inference_workspace(size_t a, size_t b, void **ptr, size_t *size) {
  if (!ptr || !size) return Status::ERROR_INVALID_PARAMETER;
  *size = std::max<size_t>(256, get_inference_workspace_size(a, b));
  return hipMalloc(ptr, *size) == hipSuccess ? Status::SUCCESS : Status::ERROR_OUT_OF_MEMORY;
}
Status ZstdBatchManager::free_inference_workspace(void *ptr) { return hipFree(ptr) == hipSuccess ? Status::SUCCESS : Status::ERROR_CUDA_ERROR; }

// (static: no dictionary, levels below ZH_DEEP_LEVEL; get_batch_device_temp_size_for covers the
// manager's level -- the deep matcher's scratch slots from ZH_DEEP_LEVEL on -- and dictionary)
size_t ZstdBatchManager::get_batch_device_temp_size(size_t count, size_t max_chunk) {
  return WsLayout(BatchShape(count, max_chunk, 1, false)).total;
}
size_t ZstdBatchManager::get_batch_device_temp_size_for(size_t count, size_t max_chunk) const {
  return WsLayout(pimpl_->device_shape(count, max_chunk)).total;
}

Status ZstdBatchManager::compress_batch_device(const void *const *d_in_ptrs, const size_t *d_in_sizes, size_t max_chunk, size_t count,
                                               void *const *d_out_ptrs, size_t *d_out_sizes, int *d_statuses, void *temp, size_t temp_size,
                                               hipStream_t stream) {
  return pimpl_->run_device({d_in_ptrs, d_in_sizes, d_out_ptrs, nullptr, nullptr, nullptr}, false, max_chunk, count, d_out_sizes, d_statuses, temp, temp_size, stream);
}

size_t ZstdBatchManager::get_batch_device_levels_temp_size(size_t count, size_t max_chunk) {
  return WsLayout(BatchShape::mixed_levels(count, max_chunk)).total;
}
Status ZstdBatchManager::compress_batch_device_levels(const void *const *d_in_ptrs, const size_t *d_in_sizes, const int *d_levels, size_t max_chunk,
                                                      size_t count, void *const *d_out_ptrs, size_t *d_out_sizes, int *d_statuses, void *temp,
                                                      size_t temp_size, hipStream_t stream) {
  return pimpl_->run_device({d_in_ptrs, d_in_sizes, d_out_ptrs, d_levels, nullptr, nullptr}, true, max_chunk, count, d_out_sizes, d_statuses, temp, temp_size, stream);
}

size_t ZstdBatchManager::get_batch_device_prefix_temp_size(size_t count, size_t max_chunk) const {
  return WsLayout(pimpl_->prefix_shape(count, max_chunk)).total;
}
Status ZstdBatchManager::compress_batch_device_prefix(const void *const *d_in_ptrs, const size_t *d_in_sizes, const void *const *d_prefix_ptrs,
                                                      const size_t *d_prefix_sizes, size_t max_chunk, size_t count, void *const *d_out_ptrs,
                                                      size_t *d_out_sizes, int *d_statuses, void *temp, size_t temp_size, hipStream_t stream) {
  if (count && (!d_prefix_ptrs || !d_prefix_sizes)) return Status::ERROR_INVALID_PARAMETER;
  return pimpl_->run_device({d_in_ptrs, d_in_sizes, d_out_ptrs, nullptr, d_prefix_ptrs, d_prefix_sizes}, false, max_chunk, count, d_out_sizes,
                            d_statuses, temp, temp_size, stream);
}

// ---- dictionary sets (zh_dictset.h) ----
class DictionarySet::Impl {
 public:
  std::shared_ptr<DictSetDev> dev = std::make_shared<DictSetDev>();
};
DictionarySet::DictionarySet() : pimpl_(new Impl) {}
DictionarySet::~DictionarySet() { (void)pimpl_->dev->uses.wait(); }  // (a manager it is still bound to keeps the memory)
size_t DictionarySet::count() const { return pimpl_->dev->count(); }
int DictionarySet::find(u32 dictionary_id) const { return pimpl_->dev->find(dictionary_id); }
Status DictionarySet::create(const dictionary::Dictionary *const *dicts, size_t count, hipStream_t stream, std::unique_ptr<DictionarySet> &out) {
  out.reset();
  if (!dicts || count < 1 || count > ZH_DICTSET_MAX) return Status::ERROR_INVALID_PARAMETER;
  std::vector<std::vector<u8>> host(count);
  std::vector<const u8 *> bufs(count);
  std::vector<size_t> sizes(count);
  for (size_t i = 0; i < count; i++) {
    const dictionary::Dictionary *const d = dicts[i];
    if (!d || !d->raw_content || d->raw_size < dictionary::MIN_DICT_SIZE || d->raw_size > dictionary::MAX_DICT_SIZE)
      return Status::ERROR_INVALID_PARAMETER;
    host[i].resize(d->raw_size);
    Status const s = copy_any(host[i].data(), d->raw_content, d->raw_size, stream);
    if (s != Status::SUCCESS) return s;
    bufs[i] = host[i].data();
    sizes[i] = d->raw_size;
  }
  std::unique_ptr<DictionarySet> set(new DictionarySet);
  Status const s = set->pimpl_->dev->build(bufs.data(), sizes.data(), count, stream);
  if (s != Status::SUCCESS) return s;
  out = std::move(set);
  return Status::SUCCESS;
}

Status ZstdBatchManager::set_dictionary_set(const DictionarySet *set) {
  std::lock_guard<std::mutex> lock(pimpl_->api_mutex);
  if (set && pimpl_->mgr_dict.e.n) return Status::ERROR_INVALID_PARAMETER;  // a dictionary is set: one or the other
  pimpl_->set = set ? set->impl().dev : nullptr;
  return Status::SUCCESS;
}
size_t ZstdBatchManager::get_batch_device_dicts_temp_size(size_t count, size_t max_chunk) const {
  return WsLayout(pimpl_->prefix_shape(count, max_chunk)).total;
}
Status ZstdBatchManager::compress_batch_device_dicts(const void *const *d_in_ptrs, const size_t *d_in_sizes, const int32_t *d_dict_index,
                                                     size_t max_chunk, size_t count, void *const *d_out_ptrs, size_t *d_out_sizes,
                                                     int *d_statuses, void *temp, size_t temp_size, hipStream_t stream) {
  if (!d_dict_index) return Status::ERROR_INVALID_PARAMETER;
  ZhPlanArrays a{d_in_ptrs, d_in_sizes, d_out_ptrs, nullptr, nullptr, nullptr};
  a.dict_index = d_dict_index;
  return pimpl_->run_device(a, false, max_chunk, count, d_out_sizes, d_statuses, temp, temp_size, stream);
}

size_t ZstdBatchManager::get_batch_device_decompress_temp_size(size_t count, size_t max_out) {
  return DecLayout::make(std::max<size_t>(1, count), max_out).total;
}

Status ZstdBatchManager::decompress_batch_device(const void *const *d_in_ptrs, const size_t *d_in_sizes, const size_t *d_out_caps, size_t max_out,
                                                 size_t count, void *const *d_out_ptrs, size_t *d_out_sizes, int *d_statuses, void *temp,
                                                 size_t temp_size, hipStream_t stream) {
  return decompress_batch_device_prefix(d_in_ptrs, d_in_sizes, nullptr, nullptr, d_out_caps, max_out, count, d_out_ptrs, d_out_sizes, d_statuses, temp,
                                        temp_size, stream);
}
// (d_prefix_sizes null: the plain entry, with the manager's dictionary if one is set)
Status ZstdBatchManager::decompress_batch_device_prefix(const void *const *d_in_ptrs, const size_t *d_in_sizes, const void *const *d_prefix_ptrs,
                                                        const size_t *d_prefix_sizes, const size_t *d_out_caps, size_t max_out, size_t count,
                                                        void *const *d_out_ptrs, size_t *d_out_sizes, int *d_statuses, void *temp,
                                                        size_t temp_size, hipStream_t stream) {
  return pimpl_->run_device_decompress(d_in_ptrs, d_in_sizes, d_prefix_ptrs, d_prefix_sizes, nullptr, d_out_caps, max_out, count, d_out_ptrs,
                                       d_out_sizes, d_statuses, temp, temp_size, stream);
}
// With a dictionary set bound every frame's dictionary is resolved on the device from its
// Dictionary_ID; d_dict_index (optional) names entries outright.
Status ZstdBatchManager::decompress_batch_device_dicts(const void *const *d_in_ptrs, const size_t *d_in_sizes, const int32_t *d_dict_index,
                                                       const size_t *d_out_caps, size_t max_out, size_t count, void *const *d_out_ptrs,
                                                       size_t *d_out_sizes, int *d_statuses, void *temp, size_t temp_size, hipStream_t stream) {
  if (!pimpl_->set) return Status::ERROR_INVALID_PARAMETER;
  return pimpl_->run_device_decompress(d_in_ptrs, d_in_sizes, nullptr, nullptr, d_dict_index, d_out_caps, max_out, count, d_out_ptrs, d_out_sizes,
                                       d_statuses, temp, temp_size, stream);
}
Status ZstdBatchManager::Impl::run_device_decompress(const void *const *d_in_ptrs, const size_t *d_in_sizes, const void *const *d_prefix_ptrs,
                                                     const size_t *d_prefix_sizes, const int32_t *d_dict_index, const size_t *d_out_caps,
                                                     size_t max_out, size_t count, void *const *d_out_ptrs, size_t *d_out_sizes, int *d_statuses,
                                                     void *temp, size_t temp_size, hipStream_t stream) {
  // one manager serialises calls (the dictionary's use events: set_dictionary waits on them)
  std::lock_guard<std::mutex> lock(api_mutex);
  Status s = ensure_kernels();
  if (s != Status::SUCCESS) return s;
  if (!count) return Status::SUCCESS;
  if (!d_in_ptrs || !d_in_sizes || !d_out_ptrs || !d_out_sizes || max_out == 0) return Status::ERROR_INVALID_PARAMETER;
  bool const prefix = d_prefix_ptrs || d_prefix_sizes;
  if (prefix && (!d_prefix_ptrs || !d_prefix_sizes || mgr_dict.e.n || set)) return Status::ERROR_INVALID_PARAMETER;
  if (d_dict_index && !set) return Status::ERROR_INVALID_PARAMETER;
  DecLayout L = DecLayout::make(count, max_out);
  if (!temp || temp_size < L.total) return Status::ERROR_BUFFER_TOO_SMALL;
  u8 *base = aligned_base(temp);
  ZhDecArgs a = L.args(base);
  mgr_dict.fill(a);
  std::shared_ptr<DictSetDev> const ds = set;
  if (ds) ds->fill(a, d_dict_index);
  a.pre_ptrs = d_prefix_ptrs;
  a.pre_sizes = d_prefix_sizes;
  a.in_ptrs = d_in_ptrs;
  a.in_sizes = d_in_sizes;
  a.out_ptrs = d_out_ptrs;
  a.out_caps = d_out_caps;
  a.out_cap_all = max_out;
  a.out_sizes = d_out_sizes;
  a.statuses = d_statuses ? (u32 *)d_statuses : (u32 *)(base + L.statuses);
  a.nvcomp_codes = 1;
  if (zh::launch_decompress(a, (u32)count, stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
  return note_dict_use(ds, stream);
}

// The decompressed size of every buffer, on the device (zh_dec_size_kernel): one launch, no
// workspace, no allocation, no synchronisation.  The manager's dictionary goes in as it does for
// decompress_batch_device (Dictionary_ID checks; a formatted one's tables serve first blocks).
Status ZstdBatchManager::get_decompressed_sizes_async(const void *const *d_ptrs, const size_t *d_sizes, size_t count, size_t *d_out_sizes,
                                                      int *d_statuses, hipStream_t stream, bool nvcomp_codes) {
  std::lock_guard<std::mutex> lock(pimpl_->api_mutex);
  Status s = ensure_kernels();
  if (s != Status::SUCCESS) return s;
  if (!count) return Status::SUCCESS;
  if (!d_ptrs || !d_sizes || !d_out_sizes || count > 0xFFFFFFFFull) return Status::ERROR_INVALID_PARAMETER;
  ZhDecArgs a{};
  pimpl_->mgr_dict.fill(a);
  std::shared_ptr<DictSetDev> const ds = pimpl_->set;  // a bound dictionary set: every frame's dictionary by its ID
  if (ds) ds->fill(a, nullptr);
  a.in_ptrs = d_ptrs;
  a.in_sizes = d_sizes;
  a.out_sizes = d_out_sizes;
  a.statuses = (u32 *)d_statuses;
  a.nvcomp_codes = nvcomp_codes ? 1u : 0u;
  if (zh::launch_decompress_sizes(a, (u32)count, stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
  return pimpl_->note_dict_use(ds, stream);
}

// ============================================================================
// factories / convenience (reference include/cuda_zstd_manager.h:358-386)
// ============================================================================
std::unique_ptr<ZstdManager> create_manager(int level) {
  if (!is_valid_compression_level(level)) throw std::invalid_argument("compression level");
  return std::unique_ptr<ZstdManager>(new ZstdBatchManager(CompressionConfig::from_level(level)));
}
std::unique_ptr<ZstdManager> create_manager(const CompressionConfig &c) { return std::unique_ptr<ZstdManager>(new ZstdBatchManager(c)); }
std::unique_ptr<ZstdBatchManager> create_batch_manager(int level) {
  return std::unique_ptr<ZstdBatchManager>(new ZstdBatchManager(CompressionConfig::from_level(level)));
}
namespace {
// one frame through a temporary manager (level, optional dictionary), workspace allocated here
Status oneshot(bool comp, const void *in, size_t n, void *out, size_t *out_size, int level, const dictionary::Dictionary *dict, hipStream_t stream) {
  if (!is_valid_compression_level(level)) return Status::ERROR_INVALID_PARAMETER;
  ZstdBatchManager m(CompressionConfig::from_level(level));
  if (dict) {
    Status const sd = m.set_dictionary(*dict);
    if (sd != Status::SUCCESS) return sd;
  }
  size_t need = comp ? m.get_compress_temp_size(n) : m.get_decompress_temp_size(n);
  void *ws = nullptr;
  if (hipMalloc(&ws, need) != hipSuccess) return Status::ERROR_OUT_OF_MEMORY;
  Status s = comp ? m.compress(in, n, out, out_size, ws, need, nullptr, 0, stream) : m.decompress(in, n, out, out_size, ws, need, stream);
  (void)hipFree(ws);
  return s;
}
}  // namespace
Status compress_simple(const void *in, size_t n, void *out, size_t *out_size, int level, hipStream_t stream) {
  return ZH_NOTED(oneshot(true, in, n, out, out_size, level, nullptr, stream));
}
Status decompress_simple(const void *in, size_t n, void *out, size_t *out_size, hipStream_t stream) {
  return ZH_NOTED(oneshot(false, in, n, out, out_size, 3, nullptr, stream));  // (the default manager's level)
}
Status compress_with_dict(const void *in, size_t n, void *out, size_t *out_size, const dictionary::Dictionary &dict, int level, hipStream_t stream) {
  return ZH_NOTED(oneshot(true, in, n, out, out_size, level, &dict, stream));
}
Status decompress_with_dict(const void *in, size_t n, void *out, size_t *out_size, const dictionary::Dictionary &dict, hipStream_t stream) {
  return ZH_NOTED(oneshot(false, in, n, out, out_size, 3, &dict, stream));
}

// reference src/cuda_zstd_types.cpp:271-560 (per-stage pool buffers) -> one region here
Status allocate_compression_workspace(CompressionWorkspace &w, size_t max_block_size, const CompressionConfig &config) {
  if (w.is_allocated || max_block_size == 0) return ZH_NOTED(Status::ERROR_INVALID_PARAMETER);
  Status const sv = config.validate();
  if (sv != Status::SUCCESS) return ZH_NOTED(sv);
  ZstdBatchManager m(config);
  size_t const need = m.get_compress_temp_size(max_block_size);
  void *p = nullptr;
  if (hipMalloc(&p, need) != hipSuccess) return ZH_NOTED(Status::ERROR_OUT_OF_MEMORY);
  w = CompressionWorkspace{};
  w.d_workspace = p;
  w.total_size = w.total_size_bytes = need;
  w.is_allocated = true;
  w.hash_table_size = 1u << config.hash_log;
  w.chain_table_size = 1u << config.chain_log;
  w.max_matches = (u32)std::min<size_t>(max_block_size, 0xFFFFFFFFu);
  w.max_costs = w.max_matches + 1;
  w.max_sequences = w.max_matches / 3;
  w.num_blocks = (u32)((max_block_size + ZH_BLOCK_MAX - 1) / ZH_BLOCK_MAX);
  return Status::SUCCESS;
}
Status free_compression_workspace(CompressionWorkspace &w) {
  Status s = Status::SUCCESS;
  if (w.d_workspace && hipFree(w.d_workspace) != hipSuccess) s = Status::ERROR_CUDA_ERROR;
  w = CompressionWorkspace{};
  return ZH_NOTED(s);
}

}  // namespace cuda_zstd

using namespace cuda_zstd;

extern "C" {
// Test hooks (tests/test_gpu_dictset.py, not product entry points): the precomputed tables of one
// dictionary copied back -- entry `index` of a set, and a host buffer loaded as set_dictionary
// loads it (DevDict::load: the same builders over a set of one, any size from 1 byte).  dtab: 2^15 u16, K1's packed
// tables (written when *P != 0); prev: ZH_DEEP_PRE u32, the deep matcher's links, [0, *split)
// written; head: 2^ZH_HASH_LOG_SHORT u32 (written when *dP != 0).  Returns 0, 1 (HIP error) or 2.
static int copy_dict_tables(const ZhDictSetEntry &e, u16 *dtab, u32 *P, u32 *prev, u32 *head, u32 *dP, u32 *split) {
  *P = e.dtab_P;
  *dP = e.dd_pre;
  *split = e.dd_split;
  size_t const tab_bytes = ((size_t(1) << ZH_HASH_LOG_LONG) + (size_t(1) << ZH_HASH_LOG_SHORT)) * 2;
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  if (e.dtab_P && hipMemcpy(dtab, e.dtab, tab_bytes, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  if (e.dd_pre && e.dd_split && hipMemcpy(prev, e.dd_prev, (size_t)e.dd_split * 4, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  if (e.dd_pre && hipMemcpy(head, e.dd_head, size_t(4) << ZH_HASH_LOG_SHORT, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  return 0;
}
int zh_test_dictset_tables(const cuda_zstd_dict_set_t *set, size_t index, u16 *dtab, u32 *P, u32 *prev, u32 *head, u32 *dP, u32 *split) {
  if (!set || !set->set || index >= set->set->count()) return 2;
  return copy_dict_tables(set->set->impl().dev->ents[index], dtab, P, prev, head, dP, split);
}
int zh_test_dict_tables(const void *buf, size_t n, u16 *dtab, u32 *P, u32 *prev, u32 *head, u32 *dP, u32 *split) {
  if (ensure_kernels() != Status::SUCCESS) return 1;
  DevDict d;
  if (d.load(buf, n, 0) != Status::SUCCESS) return 2;
  return copy_dict_tables(d.e, dtab, P, prev, head, dP, split);
}

}  // extern "C"

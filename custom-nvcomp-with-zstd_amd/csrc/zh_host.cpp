// zh_host.cpp — C++17 host runtime: managers, workspace planning, C ABI.
//
// Host side of the reference's L3/L4: ZstdBatchManager /
// NvcompV5BatchManager / HybridEngine / C API, redesigned around one batched
// device pipeline (K1 zh_lz_kernel -> K2 zh_entropy_kernel -> [K3 gather]) with a
// single host synchronisation per call instead of the reference's ~13 per block
// (src/cuda_zstd_manager.cu:2328-3112).
#include <hip/hip_runtime.h>
#include <dlfcn.h>
// AddressSanitizer refuses RTLD_DEEPBIND dlopens: sanitizer builds of the host code
// open libzstd without it
#if defined(__SANITIZE_ADDRESS__)
#define ZH_DLOPEN_DEEPBIND 0
#elif defined(__has_feature)
#if __has_feature(address_sanitizer)
#define ZH_DLOPEN_DEEPBIND 0
#endif
#endif
#ifndef ZH_DLOPEN_DEEPBIND
#define ZH_DLOPEN_DEEPBIND RTLD_DEEPBIND
#endif

#include <algorithm>
#include <chrono>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "cuda_zstd_adaptive.h"
#include "cuda_zstd_hybrid.h"
#include "cuda_zstd_manager.h"
#include "cuda_zstd_nvcomp.h"
#include "zh_adaptive.h"
#include "zh_dict.h"
#include "zh_dict_entropy.h"
#include "zh_dict_finalize.h"
#include "zh_dict_train.h"
#include "zh_launch.h"
#include "zh_seek.h"
#include "zh_stream_window.h"

namespace cuda_zstd {

// ============================================================================
// status strings (reference src/cuda_zstd_types.cpp:36-79)
// ============================================================================
const char *status_to_string(Status s) {
  switch (s) {
    case Status::SUCCESS: return "Success";
    case Status::ERROR_GENERIC: return "Generic error";
    case Status::ERROR_INVALID_PARAMETER: return "Invalid parameter";
    case Status::ERROR_OUT_OF_MEMORY: return "Out of memory";
    case Status::ERROR_CUDA_ERROR: return "HIP runtime error";
    case Status::ERROR_INVALID_MAGIC: return "Invalid magic number";
    case Status::ERROR_CORRUPT_DATA: return "Corrupt data";
    case Status::ERROR_BUFFER_TOO_SMALL: return "Buffer too small";
    case Status::ERROR_UNSUPPORTED_VERSION: return "Unsupported version";
    case Status::ERROR_DICTIONARY_MISMATCH: return "Dictionary mismatch";
    case Status::ERROR_CHECKSUM_FAILED: return "Checksum failed";
    case Status::ERROR_IO: return "I/O error";
    case Status::ERROR_COMPRESSION: return "Compression error";
    case Status::ERROR_DECOMPRESSION: return "Decompression error";
    case Status::ERROR_WORKSPACE_INVALID: return "Workspace invalid";
    case Status::ERROR_STREAM_ERROR: return "Stream error";
    case Status::ERROR_ALLOCATION_FAILED: return "Allocation failed";
    case Status::ERROR_HASH_TABLE_FULL: return "Hash table full";
    case Status::ERROR_SEQUENCE_ERROR: return "Sequence error";
    case Status::ERROR_NOT_INITIALIZED: return "Not initialized";
    case Status::ERROR_ALREADY_INITIALIZED: return "Already initialized";
    case Status::ERROR_INVALID_STATE: return "Invalid state";
    case Status::ERROR_TIMEOUT: return "Timeout";
    case Status::ERROR_CANCELLED: return "Cancelled";
    case Status::ERROR_NOT_IMPLEMENTED: return "Not implemented";
    case Status::ERROR_INTERNAL: return "Internal error";
    case Status::ERROR_UNKNOWN: return "Unknown error";
    case Status::ERROR_DICTIONARY_FAILED: return "Dictionary failed";
    case Status::ERROR_UNSUPPORTED_FORMAT: return "Unsupported format";
  }
  return "Unknown error";
}

// ============================================================================
// error context / last error (reference src/cuda_zstd_types.cpp:81-141)
// ============================================================================
namespace {
std::recursive_mutex &error_mutex() {
  static std::recursive_mutex m;
  return m;
}
ErrorContext g_last_error;
ErrorCallback g_error_callback = nullptr;
}  // namespace
const char *get_detailed_error_message(const ErrorContext &ctx) {
  static thread_local char buf[512];
  const char *const file = ctx.file ? ctx.file : "unknown", *const fn = ctx.function ? ctx.function : "unknown";
  const char *const sep = ctx.message ? " - " : "", *const msg = ctx.message ? ctx.message : "";
  if (ctx.cuda_error != hipSuccess)
    snprintf(buf, sizeof(buf), "%s at %s:%d in %s() - HIP Error: %s (%d)%s%s", status_to_string(ctx.status), file, ctx.line, fn,
             hipGetErrorString(ctx.cuda_error), (int)ctx.cuda_error, sep, msg);
  else
    snprintf(buf, sizeof(buf), "%s at %s:%d in %s()%s%s", status_to_string(ctx.status), file, ctx.line, fn, sep, msg);
  return buf;
}
void set_error_callback(ErrorCallback cb) {
  std::lock_guard<std::recursive_mutex> g(error_mutex());
  g_error_callback = cb;
}
void log_error(const ErrorContext &ctx) {
  std::lock_guard<std::recursive_mutex> g(error_mutex());
  g_last_error = ctx;
  if (g_error_callback) g_error_callback(ctx);
}
ErrorContext get_last_error() {
  std::lock_guard<std::recursive_mutex> g(error_mutex());
  return g_last_error;
}
void clear_last_error() {
  std::lock_guard<std::recursive_mutex> g(error_mutex());
  g_last_error = ErrorContext();
}
namespace {
// a public entry point's result: failures go to the last-error slot (and the callback)
inline Status noted(Status s, const char *fn, int line) {
  if (s != Status::SUCCESS) log_error(ErrorContext(s, __FILE__, line, fn));
  return s;
}
}  // namespace
#define ZH_NOTED(s) noted((s), __func__, __LINE__)

// ============================================================================
// CompressionConfig (reference src/cuda_zstd_types.cpp:147-210, 860-950)
// ============================================================================
Strategy CompressionConfig::level_to_strategy(int level) {
  if (level <= 1) return Strategy::FAST;
  if (level <= 3) return Strategy::DFAST;
  if (level <= 6) return Strategy::GREEDY;
  if (level <= 12) return Strategy::LAZY;
  if (level <= 15) return Strategy::LAZY2;
  if (level <= 18) return Strategy::BTLAZY2;
  if (level <= 20) return Strategy::BTOPT;
  return Strategy::BTULTRA;
}
int CompressionConfig::strategy_to_default_level(Strategy s) {
  switch (s) {
    case Strategy::FAST: return 1;
    case Strategy::DFAST: return 3;
    case Strategy::GREEDY: return 5;
    case Strategy::LAZY: return 9;
    case Strategy::LAZY2: return 14;
    case Strategy::BTLAZY2: return 17;
    case Strategy::BTOPT: return 19;
    default: return 22;
  }
}
void apply_level_parameters(CompressionConfig &c) {
  int level = std::min(std::max(c.level, (int)MIN_COMPRESSION_LEVEL), (int)MAX_COMPRESSION_LEVEL);
  c.strategy = CompressionConfig::level_to_strategy(level);
  c.min_match = 3;
  if (level <= 1) { c.window_log = 18; c.hash_log = 15; c.chain_log = 15; c.search_log = 1; c.target_length = 0; }
  else if (level <= 3) { c.window_log = 19; c.hash_log = 17; c.chain_log = 17; c.search_log = 1; c.target_length = 0; }
  else if (level <= 6) { c.window_log = 20; c.hash_log = 17; c.chain_log = 17; c.search_log = level == 4 ? 2 : level == 5 ? 4 : 8; c.target_length = level <= 5 ? 0 : 8; }
  else if (level <= 9) { c.window_log = 22; c.hash_log = 18; c.chain_log = 18; c.search_log = level == 7 ? 8 : level == 8 ? 16 : 32; c.target_length = level <= 8 ? 16 : 32; }
  else if (level <= 12) { c.window_log = 23; c.hash_log = 19; c.chain_log = 19; c.search_log = level == 10 ? 64 : level == 11 ? 128 : 256; c.target_length = 64; }
  else if (level <= 15) { c.window_log = 23; c.hash_log = level <= 14 ? 19 : 20; c.chain_log = 19; c.search_log = level <= 14 ? 256 : 512; c.target_length = 128; }
  else if (level <= 18) { c.window_log = 23; c.hash_log = 20; c.chain_log = 20; c.search_log = level <= 17 ? 512 : 999; c.target_length = 256; }
  else { c.window_log = 23; c.hash_log = 20; c.chain_log = 20; c.search_log = 999; c.target_length = 999; }
  // the window logs above, as the table the device shares (a mixed-level batch's frame headers)
  static_assert(ZH_LEVEL_WINDOW_LOG(1) == 18 && ZH_LEVEL_WINDOW_LOG(3) == 19 && ZH_LEVEL_WINDOW_LOG(6) == 20 && ZH_LEVEL_WINDOW_LOG(9) == 22 &&
                    ZH_LEVEL_WINDOW_LOG(10) == 23 && ZH_LEVEL_WINDOW_LOG(22) == 23,
                "one window log per level");
  c.window_log = ZH_LEVEL_WINDOW_LOG(level);
}
CompressionConfig CompressionConfig::from_level(int level) {
  CompressionConfig c;
  c.compression_mode = CompressionMode::LEVEL_BASED;
  c.level = level;
  c.use_exact_level = true;
  apply_level_parameters(c);
  return c;
}
CompressionConfig CompressionConfig::optimal(size_t) { return from_level(3); }
CompressionConfig CompressionConfig::get_default() { return from_level(3); }
Status CompressionConfig::validate() const {
  if (!is_valid_compression_level(level)) return Status::ERROR_INVALID_PARAMETER;
  if (window_log < MIN_WINDOW_LOG || window_log > MAX_WINDOW_LOG) return Status::ERROR_INVALID_PARAMETER;
  if (block_size == 0) return Status::ERROR_INVALID_PARAMETER;
  return Status::SUCCESS;
}
Status validate_config(const CompressionConfig &c) { return c.validate(); }

// reference src/cuda_zstd_types.cpp:831-853 (callers size outputs with it)
size_t estimate_compressed_size(size_t n, int) {
  size_t nb = (n + (128 * 1024 - 1)) / (128 * 1024);
  if (nb == 0) nb = 1;
  return n + n / 255 + nb * 3 + 512;
}
u32 get_optimal_block_size(u32 input_size, u32) {
  (void)input_size;
  return ZH_BLOCK_MAX;
}

ZstdManager::ExecutionPath ZstdManager::select_execution_path(size_t size, int cpu_threshold) {
  return (cpu_threshold > 0 && size < (size_t)cpu_threshold) ? ExecutionPath::CPU : ExecutionPath::GPU_BATCH;
}

// ============================================================================
// host libzstd bridge (the reference's CPU route; FORCE_CPU + decompress)
// ============================================================================
namespace {
constexpr u32 kSkippableMagic = 0x184D2A50u;  // RFC 8878 skippable frames 0x184D2A50..5F
constexpr u32 kMetadataMagic = 0x444D5A43u;   // "CZMD": this library's metadata frame
constexpr size_t kMetadataFrameBytes = 16;
struct LibZstd {
  size_t (*compress)(void *, size_t, const void *, size_t, int) = nullptr;
  size_t (*decompress)(void *, size_t, const void *, size_t) = nullptr;
  unsigned (*isError)(size_t) = nullptr;
  unsigned long long (*frameContentSize)(const void *, size_t) = nullptr;
  size_t (*compressBound)(size_t) = nullptr;
  bool ok = false;
  LibZstd() {
    const char *names[] = {"libzstd.so.1", "libzstd.so", "/opt/conda/lib/libzstd.so.1", "/usr/lib/x86_64-linux-gnu/libzstd.so.1"};
    for (const char *nm : names) {
      // RTLD_DEEPBIND: a libzstd opened here binds its own calls inside itself even when another
      // libzstd image sits in the global scope (a preloaded tool's), never mixing two versions
      void *h = dlopen(nm, RTLD_NOW | RTLD_LOCAL | ZH_DLOPEN_DEEPBIND);
      if (!h) continue;
      compress = (decltype(compress))dlsym(h, "ZSTD_compress");
      decompress = (decltype(decompress))dlsym(h, "ZSTD_decompress");
      isError = (decltype(isError))dlsym(h, "ZSTD_isError");
      frameContentSize = (decltype(frameContentSize))dlsym(h, "ZSTD_getFrameContentSize");
      compressBound = (decltype(compressBound))dlsym(h, "ZSTD_compressBound");
      ok = compress && decompress && isError && frameContentSize && compressBound;
      if (ok) break;
    }
  }
};
LibZstd &libzstd() {
  static LibZstd z;
  return z;
}

bool is_device_ptr(const void *p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

Status copy_any(void *dst, const void *src, size_t n, hipStream_t stream) {
  if (!n) return Status::SUCCESS;
  if (!is_device_ptr(dst) && !is_device_ptr(src)) {  // host to host (FORCE_CPU on host buffers): no HIP call
    memmove(dst, src, n);
    return Status::SUCCESS;
  }
  if (hipMemcpyAsync(dst, src, n, hipMemcpyDefault, stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
  if (hipStreamSynchronize(stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
  return Status::SUCCESS;
}

// reference CPU route: D2H, ZSTD_compress(level), H2D (src/cuda_zstd_manager.cu:1607-1668)
Status cpu_compress(const void *in, size_t n, void *out, size_t *out_size, int level, hipStream_t stream) {
  LibZstd &z = libzstd();
  if (!z.ok) return Status::ERROR_NOT_IMPLEMENTED;
  std::vector<u8> h_in(n), h_out(z.compressBound(n));
  Status s = copy_any(h_in.data(), in, n, stream);
  if (s != Status::SUCCESS) return s;
  size_t c = z.compress(h_out.data(), h_out.size(), h_in.data(), n, level);
  if (z.isError(c)) return Status::ERROR_COMPRESSION;
  if (c > *out_size) return Status::ERROR_BUFFER_TOO_SMALL;
  s = copy_any(out, h_out.data(), c, stream);
  if (s != Status::SUCCESS) return s;
  *out_size = c;
  return Status::SUCCESS;
}

// reference decompress CPU route (src/cuda_zstd_manager.cu:3219-3344)
Status cpu_decompress(const void *in, size_t n, void *out, size_t *out_size, hipStream_t stream) {
  LibZstd &z = libzstd();
  if (!z.ok) return Status::ERROR_NOT_IMPLEMENTED;
  if (!in || !out || !out_size || n < 4) return Status::ERROR_INVALID_PARAMETER;
  std::vector<u8> h_in(n);
  Status s = copy_any(h_in.data(), in, n, stream);
  if (s != Status::SUCCESS) return s;
  u32 magic;
  memcpy(&magic, h_in.data(), 4);
  if (magic != ZSTD_MAGIC) return Status::ERROR_INVALID_MAGIC;
  unsigned long long fcs = z.frameContentSize(h_in.data(), n);
  if (fcs == (unsigned long long)-2) return Status::ERROR_CORRUPT_DATA;
  size_t cap = *out_size;
  if (fcs != (unsigned long long)-1 && fcs > cap) return Status::ERROR_BUFFER_TOO_SMALL;
  std::vector<u8> h_out(fcs != (unsigned long long)-1 ? (size_t)fcs : cap);
  size_t d = z.decompress(h_out.data(), h_out.size(), h_in.data(), n);
  if (z.isError(d)) return Status::ERROR_CORRUPT_DATA;
  if (d > cap) return Status::ERROR_BUFFER_TOO_SMALL;
  s = copy_any(out, h_out.data(), d, stream);
  if (s != Status::SUCCESS) return s;
  *out_size = d;
  return Status::SUCCESS;
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
// A caller's temp buffer starts at its first 256-byte boundary (every layout's total holds the slack)
inline u8 *aligned_base(void *temp) { return (u8 *)align256((uintptr_t)temp); }

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
    size_t o = 0;
    auto take = [&o](size_t bytes) { size_t const at = o; o = align256(o + bytes); return at; };  // (0 bytes: an empty region)
    descs = take(nblocks * sizeof(ZhBlockDesc));
    items = take(nitems * sizeof(ZhItemDesc));
    blk_size = take(nblocks * 4);
    item_size = take(nitems * 8);
    item_status = take(nitems * 4);
    staging = take(s.staged ? nblocks * (size_t)ZH_STAGE_SLOT : 0);
    counter = take(4);
    blocks = take(nblocks * (size_t)ZH_WS_BLOCK_BYTES);
    deep_slots = s.deep ? std::min(nblocks, (size_t)ZH_DEEP_SLOTS_MAX) : 0;
    deep = take(deep_slots * ZH_DEEP_SLOT_BYTES);
    ldm_table = take(cells ? sizeof(u64) << s.ldm_tlog : 0);
    ldm_skey = take(cells * ZH_LDM_CELL_SAMPLES * sizeof(u64));
    ldm_sslot = take(cells * ZH_LDM_CELL_SAMPLES * sizeof(u32));
    ldm_scount = take(cells * sizeof(u32));
    ldm_rec = take(cells * sizeof(ZhLdmRecord));
    rank = take(s.levels ? nitems * 4 : 0);
    blk_level = take(s.levels ? nblocks : 0);
    ranges = take(s.levels ? sizeof(ZhClassRanges) : 0);
    total = o + 256;  // slack for base alignment
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
    size_t o = 0;
    L.in_ptrs = o; o = align256(o + n * 8);
    L.in_sizes = o; o = align256(o + n * 8);
    L.out_ptrs = o; o = align256(o + n * 8);
    L.caps = o; o = align256(o + n * 8);
    L.out_sizes = o; o = align256(o + n * 8);
    L.statuses = o; o = align256(o + n * 4);
    L.slots = o; o = align256(o + n * L.slot_bytes);
    L.total = o + 256;  // slack for base alignment
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

std::once_flag g_init_flag;
hipError_t g_init_err = hipSuccess;
Status ensure_kernels() {
  std::call_once(g_init_flag, [] { g_init_err = zh::init_kernels(); });
  return g_init_err == hipSuccess ? Status::SUCCESS : Status::ERROR_CUDA_ERROR;
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
    size_t o = 0;
    auto take = [&o](size_t bytes) { size_t const at = o; o = align256(o + bytes); return at; };
    size_t const o_ents = take(n * sizeof(ZhDictSetEntry)), o_ids = take(n * sizeof(ZhDictSetId)), o_jobs = take(n * sizeof(ZhDictBuildJob));
    std::vector<size_t> o_buf(n), o_dent(n, 0), o_dtab(n, 0), o_prev(n, 0), o_head(n, 0);
    std::vector<ZhDictEnt> blobs(n);
    std::vector<u8> has_ent(n, 0);
    for (size_t i = 0; i < n; i++) {
      o_buf[i] = take(sizes[i]);
      // a formatted dictionary: its Huffman code, FSE encoding tables, bit costs and repcodes
      // (none for a section the encoder cannot use)
      size_t co2 = 0;
      if (offs[i] && zh::dent::parse(bufs[i], sizes[i], &blobs[i], &co2) && co2 == offs[i]) {
        has_ent[i] = 1;
        o_dent[i] = take(sizeof(ZhDictEnt));
      }
    }
    size_t const upload = o;
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
      if (e.dtab_P) o_dtab[i] = take(tab_entries * 2);
      if (e.dd_pre) {
        o_prev[i] = take((size_t)e.dd_split * 4);
        o_head[i] = take(size_t(4) << ZH_HASH_LOG_SHORT);
      }
    }
    mem_bytes = o;
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
}  // namespace

// ============================================================================
// ZstdBatchManager
// ============================================================================
class ZstdBatchManager::Impl {
 public:
  CompressionConfig config;
  CompressionStats stats;
  dictionary::DictionaryHeader dict_hdr{};  // set_dictionary's header (dictionary_id: the frames' RFC ID)
  bool has_dict = false;
  std::mutex api_mutex;  // one manager serialises calls (reference src/cuda_zstd_manager.cu:1542)
  void *pinned = nullptr;
  size_t pinned_bytes = 0;
  DevDict mgr_dict, call_dict;  // set_dictionary()'s / compress()'s per-call dictionary
  u32 *stats_dev = nullptr;     // collect_entropy_stats: run() asks the entropy kernel for its histograms (ZH_F_STATS)
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
    if (ds) return ds->uses.note(stream);
    return dd ? dd->note_use(stream) : Status::SUCCESS;
  }

  // The device-array decoding entries (defined with them below): prefixes, or the bound dictionary
  // set with an optional entry index per buffer
  Status run_device_decompress(const void *const *d_in_ptrs, const size_t *d_in_sizes, const void *const *d_prefix_ptrs,
                               const size_t *d_prefix_sizes, const int32_t *d_dict_index, const size_t *d_out_caps, size_t max_out, size_t count,
                               void *const *d_out_ptrs, size_t *d_out_sizes, int *d_statuses, void *temp, size_t temp_size, hipStream_t stream);

  // Run the device pipeline over a list of frames given as host arrays.
  // out_sizes: in = capacity, out = bytes; statuses out.
  Status run(const void *const *in_ptrs, const size_t *in_sizes, size_t count, void *const *out_ptrs, size_t *out_sizes, Status *statuses,
             void *temp, size_t temp_size, hipStream_t stream, const DevDict *dd = nullptr, bool allow_ldm = false) {
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
    pimpl_->stats_dev = (u32 *)(buf + stats_off);
    s = pimpl_->run(d_ptrs, isz.data(), count, op.data(), osz.data(), st.data(), buf + temp_off, temp_bytes, stream, pimpl_->active());
    pimpl_->stats_dev = nullptr;
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
  auto t0 = std::chrono::steady_clock::now();
  Status st;
  if (!dd && select_execution_path(n, (int)pimpl_->config.cpu_threshold) == ExecutionPath::CPU) {
    st = cpu_compress(in, n, out, out_size, pimpl_->config.level, stream);
    if (st == Status::SUCCESS) { pimpl_->stats.input_bytes += n; pimpl_->stats.output_bytes += *out_size; }
  } else {
    Status item;
    const void *ip[1] = {in};
    void *opv[1] = {out};
    size_t sz[1] = {n};
    st = pimpl_->run(ip, sz, 1, opv, out_size, &item, temp, temp_size, stream, dd, true);
    if (st == Status::ERROR_GENERIC) st = item;
  }
  pimpl_->stats.compression_time_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
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
  auto t0 = std::chrono::steady_clock::now();
  size_t got = 0;
  Status s = pimpl_->run_decompress_one(in, n, out, *out_size, &got, nullptr, temp, temp_size, stream);
  if (s == Status::SUCCESS) *out_size = got;
  pimpl_->stats.decompression_time_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return s;
}

Status ZstdBatchManager::compress_with_history(const void *in, size_t n, void *out, size_t *out_size, void *temp, size_t temp_size,
                                               const void *hist, size_t hist_n, hipStream_t stream) {
  std::lock_guard<std::mutex> lock(pimpl_->api_mutex);
  if (!in || !out || !out_size || !temp || (hist_n && !hist)) return Status::ERROR_INVALID_PARAMETER;
  if (n == 0) { *out_size = 0; return Status::ERROR_INVALID_PARAMETER; }
  if (temp_size < get_compress_temp_size(n)) return Status::ERROR_BUFFER_TOO_SMALL;
  DevDict view;
  if (hist_n) DevDict::view(view, hist, hist_n);
  Status item;
  const void *ip[1] = {in};
  void *opv[1] = {out};
  size_t sz[1] = {n};
  auto t0 = std::chrono::steady_clock::now();
  Status st = pimpl_->run(ip, sz, 1, opv, out_size, &item, temp, temp_size, stream, hist_n ? &view : pimpl_->active(), true);
  if (st == Status::ERROR_GENERIC) st = item;
  pimpl_->stats.compression_time_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return st;
}
Status ZstdBatchManager::decompress_with_history(const void *in, size_t n, void *out, size_t *out_size, void *temp, size_t temp_size,
                                                 const void *hist, size_t hist_n, hipStream_t stream) {
  std::lock_guard<std::mutex> lock(pimpl_->api_mutex);
  if (!in || !out || !out_size || !temp || n < 4 || (hist_n && !hist)) return Status::ERROR_INVALID_PARAMETER;
  if (temp_size < DecLayout::make(1, *out_size).total) return Status::ERROR_BUFFER_TOO_SMALL;
  DevDict view;
  if (hist_n) DevDict::view(view, hist, hist_n);
  size_t got = 0;
  Status s = pimpl_->run_decompress_one(in, n, out, *out_size, &got, nullptr, temp, temp_size, stream, hist_n ? &view : nullptr);
  if (s == Status::SUCCESS) *out_size = got;
  return s;
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
  pimpl_->has_dict = true;
  return Status::SUCCESS;
}
// reference :3858-3863: no dictionary -> ERROR_INVALID_PARAMETER; else a deep copy (the caller
// frees dict.raw_content with free(), Dictionary's copy semantics)
Status ZstdBatchManager::get_dictionary(dictionary::Dictionary &d) const {
  std::lock_guard<std::mutex> lock(pimpl_->api_mutex);  // set_dictionary swaps mgr_dict under it
  if (!pimpl_->has_dict) return Status::ERROR_INVALID_PARAMETER;
  dictionary::Dictionary view;
  view.header = pimpl_->dict_hdr;
  view.raw_content = pimpl_->mgr_dict.host.data();
  view.raw_size = (u32)pimpl_->mgr_dict.host.size();
  d = view;
  return d.raw_content ? Status::SUCCESS : Status::ERROR_OUT_OF_MEMORY;
}
Status ZstdBatchManager::clear_dictionary() {
  std::lock_guard<std::mutex> lock(pimpl_->api_mutex);
  pimpl_->has_dict = false;
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
  auto &mut = const_cast<std::vector<BatchItem> &>(items);  // reference writes sizes/status through const (:5745)
  std::vector<size_t> sizes(items.size());
  for (size_t i = 0; i < items.size(); i++) sizes[i] = items[i].input_size;
  if (temp_size < get_batch_compress_temp_size(sizes)) return Status::ERROR_BUFFER_TOO_SMALL;
  // items with invalid arguments never reach the device; the reference's batch loop calls
  // compress() per item (src/cuda_zstd_manager.cu:5744-5768), so an item below cpu_threshold
  // takes compress()'s libzstd route (without a dictionary, as compress() decides) and the rest
  // share one device launch
  const DevDict *dd = pimpl_->active();
  std::vector<const void *> ip;
  std::vector<void *> op;
  std::vector<size_t> isz, osz, idx;
  bool any_bad = false;
  auto t0 = std::chrono::steady_clock::now();
  for (size_t i = 0; i < items.size(); i++) {
    if (!items[i].input_ptr || !items[i].output_ptr || items[i].input_size == 0) {
      mut[i].status = Status::ERROR_INVALID_PARAMETER;
      any_bad = true;
      continue;
    }
    if (!dd && select_execution_path(items[i].input_size, (int)pimpl_->config.cpu_threshold) == ExecutionPath::CPU) {
      size_t o = items[i].output_size;
      mut[i].status = cpu_compress(items[i].input_ptr, items[i].input_size, items[i].output_ptr, &o, pimpl_->config.level, stream);
      if (mut[i].status == Status::SUCCESS) {
        mut[i].output_size = o;
        pimpl_->stats.input_bytes += items[i].input_size;
        pimpl_->stats.output_bytes += o;
      } else {
        any_bad = true;
      }
      continue;
    }
    ip.push_back(items[i].input_ptr);
    op.push_back(items[i].output_ptr);
    isz.push_back(items[i].input_size);
    osz.push_back(items[i].output_size);
    idx.push_back(i);
  }
  std::vector<Status> st(idx.size());
  Status r = idx.empty() ? Status::SUCCESS : pimpl_->run(ip.data(), isz.data(), idx.size(), op.data(), osz.data(), st.data(), temp, temp_size, stream, dd);
  pimpl_->stats.compression_time_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (r != Status::SUCCESS && r != Status::ERROR_GENERIC) return r;
  for (size_t j = 0; j < idx.size(); j++) {
    mut[idx[j]].status = st[j];
    if (st[j] == Status::SUCCESS) mut[idx[j]].output_size = osz[j];
    else any_bad = true;
  }
  return any_bad ? Status::ERROR_GENERIC : Status::SUCCESS;
}

// ZstdBatchManager::decompress_batch (reference src/cuda_zstd_manager.cu:5799-5885): every
// item decoded by one launch; output_size in = capacity, out = bytes; per-item status.
Status ZstdBatchManager::decompress_batch(const std::vector<BatchItem> &items, void *temp, size_t temp_size, hipStream_t stream) {
  std::lock_guard<std::mutex> lock(pimpl_->api_mutex);
  if (items.empty()) return Status::SUCCESS;
  auto &mut = const_cast<std::vector<BatchItem> &>(items);  // the reference writes sizes/status through const
  std::vector<const void *> ip;
  std::vector<void *> op;
  std::vector<size_t> isz, osz, idx;
  bool any_bad = false;
  for (size_t i = 0; i < items.size(); i++) {
    if (!items[i].input_ptr || !items[i].output_ptr || items[i].input_size < 4) {
      mut[i].status = Status::ERROR_INVALID_PARAMETER;
      any_bad = true;
      continue;
    }
    ip.push_back(items[i].input_ptr);
    op.push_back(items[i].output_ptr);
    isz.push_back(items[i].input_size);
    osz.push_back(items[i].output_size);
    idx.push_back(i);
  }
  if (idx.empty()) return Status::ERROR_GENERIC;
  auto t0 = std::chrono::steady_clock::now();
  std::vector<Status> st(idx.size());
  Status r = pimpl_->run_decompress(ip.data(), isz.data(), idx.size(), op.data(), osz.data(), st.data(), temp, temp_size, stream);
  pimpl_->stats.decompression_time_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (r != Status::SUCCESS && r != Status::ERROR_GENERIC) return r;
  for (size_t j = 0; j < idx.size(); j++) {
    mut[idx[j]].status = st[j];
    if (st[j] == Status::SUCCESS) mut[idx[j]].output_size = osz[j];
    else any_bad = true;
  }
  return any_bad ? Status::ERROR_GENERIC : Status::SUCCESS;
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
  Impl *const pimpl_ = this;
  // one manager serialises calls (the dictionary's use events: set_dictionary waits on them)
  std::lock_guard<std::mutex> lock(pimpl_->api_mutex);
  Status s = ensure_kernels();
  if (s != Status::SUCCESS) return s;
  if (!count) return Status::SUCCESS;
  if (!d_in_ptrs || !d_in_sizes || !d_out_ptrs || !d_out_sizes || max_out == 0) return Status::ERROR_INVALID_PARAMETER;
  bool const prefix = d_prefix_ptrs || d_prefix_sizes;
  if (prefix && (!d_prefix_ptrs || !d_prefix_sizes || pimpl_->mgr_dict.e.n || pimpl_->set)) return Status::ERROR_INVALID_PARAMETER;
  if (d_dict_index && !pimpl_->set) return Status::ERROR_INVALID_PARAMETER;
  DecLayout L = DecLayout::make(count, max_out);
  if (!temp || temp_size < L.total) return Status::ERROR_BUFFER_TOO_SMALL;
  u8 *base = aligned_base(temp);
  ZhDecArgs a = L.args(base);
  pimpl_->mgr_dict.fill(a);
  std::shared_ptr<DictSetDev> const ds = pimpl_->set;
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
  if (ds) return ds->uses.note(stream);
  return pimpl_->mgr_dict.e.n ? pimpl_->mgr_dict.note_use(stream) : Status::SUCCESS;
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
  if (ds) return ds->uses.note(stream);
  return pimpl_->mgr_dict.e.n ? pimpl_->mgr_dict.note_use(stream) : Status::SUCCESS;
}

// ============================================================================
// Streaming manager (reference src/cuda_zstd_manager.cu:6043-6455).  compress_chunk: each chunk
// an independent frame (:6306-6310).  compress_chunk_with_history: the chunk is compressed with
// the preceding stream bytes (a 64 KiB device window, the most K1 can stage) as raw-content
// history, as the reference passes its window to compress() as a dictionary (:6327-6418).
// decompress_chunk keeps the same window of decoded bytes and hands it to the decoder, so
// chunks of either kind decode in stream order.
// ============================================================================
namespace {
struct FrameProbe {
  u64 content = 0;
  bool has_content = false, checksum = false;
  u32 dict_id = 0, window_log = 0;
  int meta_level = -1;
  size_t frame_offset = 0;
};
Status probe_frame(const void *data, size_t n, FrameProbe &f);
constexpr size_t kStreamWindow = 64 * 1024;
// a device window of the last kStreamWindow stream bytes (double-buffered: no overlapping copies)
struct HistWindow {
  u8 *buf[2] = {nullptr, nullptr};
  int cur = 0;
  size_t n = 0;
  ~HistWindow() {
    for (u8 *b : buf)
      if (b) (void)hipFree(b);
  }
  Status ensure() {
    for (u8 *&b : buf)
      if (!b && hipMalloc(&b, kStreamWindow) != hipSuccess) { b = nullptr; return Status::ERROR_OUT_OF_MEMORY; }
    return Status::SUCCESS;
  }
  const u8 *data() const { return buf[cur]; }
  // Enqueue the window's next state (its last bytes + src) into the other buffer on `stream`,
  // without waiting: the chunk call's own stream synchronisation (its compress / decompress,
  // which is blocking on return) covers it.  The current buffer stays valid until commit().
  size_t pend_n = 0;
  Status stage(const void *src, size_t len, hipStream_t stream) {
    Status s = ensure();
    if (s != Status::SUCCESS) return s;
    u8 *const dst = buf[cur ^ 1];
    size_t const take = std::min(len, kStreamWindow), keep = std::min(n, kStreamWindow - take);
    if (keep && hipMemcpyAsync(dst, buf[cur] + n - keep, keep, hipMemcpyDeviceToDevice, stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
    if (hipMemcpyAsync(dst + keep, (const u8 *)src + len - take, take, hipMemcpyDefault, stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
    pend_n = keep + take;
    return Status::SUCCESS;
  }
  void commit() {
    cur ^= 1;
    n = pend_n;
  }
  // stage + a wait of its own (decompress_chunk: the window takes the decoded bytes, which exist
  // only after the call's synchronisation)
  Status append(const void *src, size_t len, hipStream_t stream) {
    Status s = stage(src, len, stream);
    if (s != Status::SUCCESS) return s;
    if (hipStreamSynchronize(stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
    commit();
    return Status::SUCCESS;
  }
  void clear() { n = 0; }
};
}  // namespace

class ZstdStreamingManager::Impl {
 public:
  CompressionConfig config;
  ZstdBatchManager mgr;
  void *ws = nullptr;
  size_t ws_size = 0;
  bool comp = false, decomp = false;
  HistWindow chist, dhist;  // compressor's and decompressor's stream windows
  // the session compresses chunks against the stream history (init_compression_with_history /
  // compress_chunk_with_history): decompress_chunk then decodes against the decoded window;
  // otherwise chunks are frames of their own and decode with the manager's dictionary, if any
  bool hist_mode = false;
  bool has_dict = false;  // set_dictionary succeeded (frames with its Dictionary_ID decode with it)
  explicit Impl(const CompressionConfig &c) : config(c), mgr(c) {}
  ~Impl() { if (ws) (void)hipFree(ws); }
  Status ensure_ws(size_t need) {
    if (need <= ws_size) return Status::SUCCESS;
    if (ws) (void)hipFree(ws);
    ws = nullptr;
    ws_size = 0;
    if (hipMalloc(&ws, need) != hipSuccess) return Status::ERROR_OUT_OF_MEMORY;
    ws_size = need;
    return Status::SUCCESS;
  }
};
ZstdStreamingManager::ZstdStreamingManager() : pimpl_(new Impl(CompressionConfig::from_level(3))) {}
ZstdStreamingManager::ZstdStreamingManager(const CompressionConfig &c) : pimpl_(new Impl(c)) {}
ZstdStreamingManager::~ZstdStreamingManager() = default;
Status ZstdStreamingManager::init_compression(hipStream_t, size_t max_chunk) {
  Status s = pimpl_->ensure_ws(pimpl_->mgr.get_compress_temp_size(max_chunk ? max_chunk : (size_t)ZH_BLOCK_MAX));
  if (s != Status::SUCCESS) return s;
  pimpl_->comp = true;
  return Status::SUCCESS;
}
Status ZstdStreamingManager::init_compression_with_history(hipStream_t st, size_t m) {
  Status s = init_compression(st, m);
  if (s == Status::SUCCESS) s = pimpl_->chist.ensure();
  if (s == Status::SUCCESS) pimpl_->hist_mode = true;
  return s;
}
Status ZstdStreamingManager::init_decompression_with_history(hipStream_t st) {
  Status s = init_decompression(st);
  if (s == Status::SUCCESS) pimpl_->hist_mode = true;
  return s;
}
Status ZstdStreamingManager::init_decompression(hipStream_t) {
  Status s = pimpl_->ensure_ws(pimpl_->mgr.get_decompress_temp_size(0));
  if (s == Status::SUCCESS) s = pimpl_->dhist.ensure();
  if (s != Status::SUCCESS) return s;
  pimpl_->decomp = true;
  return Status::SUCCESS;
}
Status ZstdStreamingManager::compress_chunk(const void *in, size_t n, void *out, size_t *out_size, bool, hipStream_t stream) {
  if (!pimpl_->comp) return Status::ERROR_NOT_INITIALIZED;
  Status s = pimpl_->ensure_ws(pimpl_->mgr.get_compress_temp_size(n));
  if (s != Status::SUCCESS) return s;
  // the stream window follows every chunk, so a later chunk_with_history sees these bytes (the
  // window copy is enqueued first: compress()'s final synchronisation covers it)
  bool const win = pimpl_->chist.buf[0] != nullptr;
  if (win) {
    s = pimpl_->chist.stage(in, n, stream);
    if (s != Status::SUCCESS) return s;
  }
  s = pimpl_->mgr.compress(in, n, out, out_size, pimpl_->ws, pimpl_->ws_size, nullptr, 0, stream);
  if (s == Status::SUCCESS && win) pimpl_->chist.commit();
  else if (win) (void)hipStreamSynchronize(stream);  // (an early error return: the copy still reads `in`)
  return s;
}
Status ZstdStreamingManager::compress_chunk_with_history(const void *in, size_t n, void *out, size_t *out_size, bool, hipStream_t stream) {
  if (!in || !out || !out_size) return Status::ERROR_INVALID_PARAMETER;
  if (!pimpl_->comp || !pimpl_->chist.buf[0]) {  // auto-initialise, as the reference does
    Status s = init_compression_with_history(stream, n);
    if (s != Status::SUCCESS) return s;
  }
  Status s = pimpl_->ensure_ws(pimpl_->mgr.get_compress_temp_size(n));
  if (s != Status::SUCCESS) return s;
  // the next window state goes to the other buffer while this chunk reads the current one;
  // compress_with_history's synchronisation covers the copy
  s = pimpl_->chist.stage(in, n, stream);
  if (s != Status::SUCCESS) return s;
  s = pimpl_->mgr.compress_with_history(in, n, out, out_size, pimpl_->ws, pimpl_->ws_size, pimpl_->chist.data(), pimpl_->chist.n, stream);
  if (s == Status::SUCCESS) pimpl_->chist.commit();
  else (void)hipStreamSynchronize(stream);  // (an early error return: the copy still reads `in`)
  return s;
}
Status ZstdStreamingManager::decompress_chunk(const void *in, size_t n, void *out, size_t *out_size, bool *is_last, hipStream_t stream) {
  if (!in || !out || !out_size) return Status::ERROR_INVALID_PARAMETER;
  if (!pimpl_->decomp) {
    Status s = init_decompression(stream);
    if (s != Status::SUCCESS) return s;
  }
  if (is_last) *is_last = true;  // every chunk is a complete frame
  Status s = pimpl_->ensure_ws(pimpl_->mgr.get_decompress_temp_size(n));
  if (s != Status::SUCCESS) return s;
  // Per frame: the decoded window is the frame's history unless the frame was compressed with
  // the manager's dictionary.  Without a dictionary the window is harmless (a frame of its own
  // never reaches before its start).  With one, only a history session (compression with history
  // in this manager, or init_decompression_with_history) has history frames, and those carry no
  // Dictionary_ID: a frame naming the dictionary, or any frame outside a history session -- a
  // formatted dictionary's frame written without its ID (libzstd dictIDFlag 0) included -- decodes
  // with the dictionary.  History frames therefore need init_decompression_with_history (ADVICE
  // r5): outside a history session an ID-less frame that fails against the dictionary (corrupt, or
  // its content checksum does not hold) is decoded once more against the window; an ID-less frame
  // without a checksum that decodes against the dictionary cannot be told apart and is kept.
  bool hist_frame = true, retry_hist = false;
  if (pimpl_->has_dict) {
    FrameProbe fp;
    bool const probed = probe_frame(in, n, fp) == Status::SUCCESS;
    hist_frame = pimpl_->hist_mode && probed && fp.dict_id == 0;
    retry_hist = !pimpl_->hist_mode && probed && fp.dict_id == 0 && pimpl_->dhist.n;
  }
  bool const use_hist = pimpl_->dhist.n && hist_frame;
  size_t const cap = *out_size;
  s = pimpl_->mgr.decompress_with_history(in, n, out, out_size, pimpl_->ws, pimpl_->ws_size, use_hist ? pimpl_->dhist.data() : nullptr,
                                          use_hist ? pimpl_->dhist.n : 0, stream);
  if ((s == Status::ERROR_CHECKSUM_FAILED || s == Status::ERROR_CORRUPT_DATA) && retry_hist) {
    *out_size = cap;
    s = pimpl_->mgr.decompress_with_history(in, n, out, out_size, pimpl_->ws, pimpl_->ws_size, pimpl_->dhist.data(), pimpl_->dhist.n, stream);
  }
  if (s == Status::SUCCESS) s = pimpl_->dhist.append(out, *out_size, stream);
  return s;
}
Status ZstdStreamingManager::reset() {
  pimpl_->comp = pimpl_->decomp = false;
  pimpl_->hist_mode = false;
  pimpl_->chist.clear();
  pimpl_->dhist.clear();
  return Status::SUCCESS;
}
Status ZstdStreamingManager::reset_streaming() {
  pimpl_->chist.clear();
  pimpl_->dhist.clear();
  return Status::SUCCESS;
}
Status ZstdStreamingManager::flush(hipStream_t s) { return hipStreamSynchronize(s) == hipSuccess ? Status::SUCCESS : Status::ERROR_CUDA_ERROR; }
Status ZstdStreamingManager::flush_streaming(hipStream_t s) { return flush(s); }
Status ZstdStreamingManager::set_config(const CompressionConfig &c) { pimpl_->config = c; return pimpl_->mgr.configure(c); }
Status ZstdStreamingManager::set_dictionary(const dictionary::Dictionary &d) {
  Status const s = pimpl_->mgr.set_dictionary(d);
  if (s == Status::SUCCESS) pimpl_->has_dict = true;
  return s;
}
CompressionConfig ZstdStreamingManager::get_config() const { return pimpl_->config; }
size_t ZstdStreamingManager::get_temp_size() const { return pimpl_->ws_size; }
bool ZstdStreamingManager::is_compression_initialized() const { return pimpl_->comp; }
bool ZstdStreamingManager::is_decompression_initialized() const { return pimpl_->decomp; }

// ============================================================================
// dictionary training API (reference include/cuda_zstd_dictionary.h:176-210,
// src/cuda_zstd_dictionary.cu:421-520): COVER (zh_dict.cpp) instead of the reference's
// byte-frequency / 4-gram fill, same validation and buffer contract
// ============================================================================
namespace dictionary {
namespace {
bool g_train_profile = false;  // cuda_zstd_hip_dict_train_profile: HIP events around the device trainer's kernel groups
float g_train_phase_ms[3] = {0.f, 0.f, 0.f};

// The device trainer (zh_dict_train.hip) over samples back to back at d_corpus, one dictionary per
// group of counts[g] consecutive samples; sizes and counts are host arrays.  temp == nullptr: the
// function's own hipMalloc.  contents[g] = zh::cover_train's bytes for group g's samples alone
// (none where the group has fewer than k bytes: the host trainer's empty result).
Status train_groups_device(const u8 *d_corpus, const size_t *sizes, size_t n, const size_t *counts, size_t ng, size_t dict_size, u32 k, u32 d,
                           void *temp, size_t temp_bytes, bool own_temp, hipStream_t stream, std::vector<std::vector<u8>> &contents) {
  contents.clear();
  if (!d_corpus || !sizes || !counts || n == 0 || n >= (1ull << 32) || ng == 0 || ng > zh::kCoverMaxGroups) return Status::ERROR_INVALID_PARAMETER;
  contents.resize(ng);
  k = k ? k : zh::kCoverDefaultK;
  d = d ? d : zh::kCoverDefaultD;
  size_t counted = 0;
  for (size_t g = 0; g < ng; g++) {
    if (counts[g] > n - counted) return Status::ERROR_INVALID_PARAMETER;
    counted += counts[g];
  }
  if (counted != n) return Status::ERROR_INVALID_PARAMETER;
  std::vector<u32> ends(n);
  u64 total = 0;
  for (size_t i = 0; i < n; i++) {
    total += sizes[i];
    if (sizes[i] >= (1ull << 32) || total >= (1ull << 32) - 64) return Status::ERROR_INVALID_PARAMETER;  // positions are u32
    ends[i] = (u32)total;
  }
  if (total == 0) return Status::ERROR_INVALID_PARAMETER;
  std::vector<zh::CoverGroup> groups(ng);
  (void)zh::cover_groups(sizes, counts, ng, dict_size, k, d, groups.data());
  if (groups[0].plan.k > zh::kCoverMaxK) return Status::ERROR_INVALID_PARAMETER;  // prevdist is a u16
  size_t const need = zh::cover_temp_bytes(sizes, n, counts, ng, dict_size, k);
  if (!own_temp && (!temp || temp_bytes < need)) return Status::ERROR_BUFFER_TOO_SMALL;
  bool any = false;
  for (auto const &g : groups) any = any || !g.plan.empty;
  if (!any) return Status::SUCCESS;
  void *mine = nullptr;
  if (own_temp) {
    if (hipMalloc(&mine, need) != hipSuccess) { (void)hipGetLastError(); return Status::ERROR_OUT_OF_MEMORY; }
    temp = mine;
  }
  hipError_t const e = zh::cover_train_groups_device(d_corpus, ends.data(), n, groups.data(), ng, dict_size, temp, stream, contents,
                                                     g_train_profile ? g_train_phase_ms : nullptr);
  if (mine) (void)hipFree(mine);
  if (e != hipSuccess) { (void)hipGetLastError(); return Status::ERROR_CUDA_ERROR; }
  return Status::SUCCESS;
}

// one dictionary from all samples: the call with one group
Status train_device(const u8 *d_corpus, const size_t *sizes, size_t n, size_t dict_size, u32 k, u32 d, void *temp, size_t temp_bytes,
                    bool own_temp, hipStream_t stream, std::vector<u8> &content) {
  content.clear();
  std::vector<std::vector<u8>> c;
  Status const st = train_groups_device(d_corpus, sizes, n, &n, 1, dict_size, k, d, temp, temp_bytes, own_temp, stream, c);
  if (st == Status::SUCCESS) content = std::move(c[0]);
  return st;
}

// trained content -> the dict_size bytes of dict_buffer (host or device memory)
Status place_content(const std::vector<u8> &c, void *dict_buffer, size_t dict_size, hipStream_t stream) {
  if (c.empty() || c.size() > dict_size) return Status::ERROR_DICTIONARY_FAILED;
  // the buffer holds dict_size bytes: the trained content at its end (the most useful segments
  // nearest the data, as ZDICT lays them out), zeros before it when the samples gave less
  if (!is_device_ptr(dict_buffer)) {
    u8 *const out = (u8 *)dict_buffer;
    memset(out, 0, dict_size - c.size());
    memcpy(out + dict_size - c.size(), c.data(), c.size());
    return Status::SUCCESS;
  }
  std::vector<u8> full(dict_size, 0);
  memcpy(full.data() + dict_size - c.size(), c.data(), c.size());
  return copy_any(dict_buffer, full.data(), dict_size, stream);
}
}  // namespace

Status train_dictionary(const std::vector<const void *> &samples, const std::vector<size_t> &sample_sizes, void *dict_buffer,
                        size_t dict_size, const DictionaryTrainingParams *params, hipStream_t stream) {
  if (samples.empty() || sample_sizes.empty() || !dict_buffer || samples.size() != sample_sizes.size()) return Status::ERROR_INVALID_PARAMETER;
  if (!is_valid_dictionary_size(dict_size)) return Status::ERROR_INVALID_PARAMETER;
  std::vector<std::pair<const u8 *, size_t>> s;
  size_t total = 0;
  const void *first = nullptr;
  for (size_t i = 0; i < samples.size(); i++) {
    if (!samples[i] && sample_sizes[i]) return Status::ERROR_INVALID_PARAMETER;
    s.emplace_back((const u8 *)samples[i], sample_sizes[i]);
    total += sample_sizes[i];
    if (!first && sample_sizes[i]) first = samples[i];
  }
  if (total == 0) return Status::ERROR_INVALID_PARAMETER;
  std::vector<u8> c;
  try {
    if (is_device_ptr(first)) {  // device samples (all of them): trained in place, or on the host when use_gpu is off
      bool const on_gpu = !params || params->use_gpu;
      bool contiguous = true;
      const u8 *at = (const u8 *)first;
      for (auto const &p : s) {
        if (!p.second) continue;
        contiguous = contiguous && p.first == at;
        at += p.second;
      }
      if (on_gpu && contiguous) {
        Status const st = train_device((const u8 *)first, sample_sizes.data(), samples.size(), dict_size, 0, 0, nullptr, 0, true, stream, c);
        if (st != Status::SUCCESS) return st;
      } else if (on_gpu) {
        u8 *gathered = nullptr;
        if (hipMalloc((void **)&gathered, total) != hipSuccess) { (void)hipGetLastError(); return Status::ERROR_OUT_OF_MEMORY; }
        size_t o = 0;
        hipError_t e = hipSuccess;
        for (auto const &p : s) {
          if (p.second && e == hipSuccess) e = hipMemcpyAsync(gathered + o, p.first, p.second, hipMemcpyDeviceToDevice, stream);
          o += p.second;
        }
        Status st = e == hipSuccess ? Status::SUCCESS : Status::ERROR_CUDA_ERROR;
        if (st == Status::SUCCESS) st = train_device(gathered, sample_sizes.data(), samples.size(), dict_size, 0, 0, nullptr, 0, true, stream, c);
        else (void)hipStreamSynchronize(stream);
        (void)hipFree(gathered);
        if (st != Status::SUCCESS) return st;
      } else {
        std::vector<u8> host(total);
        size_t o = 0;
        for (auto &p : s) {
          if (p.second && hipMemcpyAsync(host.data() + o, p.first, p.second, hipMemcpyDeviceToHost, stream) != hipSuccess) {
            (void)hipStreamSynchronize(stream);
            return Status::ERROR_CUDA_ERROR;
          }
          p.first = host.data() + o;
          o += p.second;
        }
        if (hipStreamSynchronize(stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
        c = zh::cover_train(s, dict_size);
      }
    } else {
      c = zh::cover_train(s, dict_size);  // host samples, whatever use_gpu says
    }
  } catch (...) {
    return Status::ERROR_OUT_OF_MEMORY;
  }
  return place_content(c, dict_buffer, dict_size, stream);
}
Status create_dictionary_from_samples(const void *samples_buffer, const size_t *sample_offsets, size_t num_samples, void *dict_buffer,
                                      size_t dict_size, const DictionaryTrainingParams *params, hipStream_t stream) {
  if (!samples_buffer || !sample_offsets || !dict_buffer || num_samples == 0) return Status::ERROR_INVALID_PARAMETER;
  std::vector<const void *> samples;
  std::vector<size_t> sizes;
  const u8 *const base = (const u8 *)samples_buffer;
  for (size_t i = 0; i < num_samples; i++) {
    size_t const a = sample_offsets[i], e = i + 1 < num_samples ? sample_offsets[i + 1] : a + 8 * 1024;
    if (e < a) return Status::ERROR_INVALID_PARAMETER;
    samples.push_back(base + a);
    sizes.push_back(e - a);
  }
  return train_dictionary(samples, sizes, dict_buffer, dict_size, params, stream);
}
Status finalize_dictionary(const void *content, size_t content_size, const std::vector<const void *> &samples,
                           const std::vector<size_t> &sample_sizes, int level, u32 dict_id, void *out, size_t *out_size, hipStream_t stream) {
  if (!content || !out || !out_size || samples.empty() || samples.size() != sample_sizes.size()) return Status::ERROR_INVALID_PARAMETER;
  if (content_size < MIN_DICT_SIZE || content_size > MAX_DICT_SIZE || !is_valid_compression_level(level)) return Status::ERROR_INVALID_PARAMETER;
  std::vector<u8> c(content_size);
  Status s = copy_any(c.data(), content, content_size, stream);
  if (s != Status::SUCCESS) return s;
  u32 id0 = 0;
  size_t co = 0;
  if (!zh::dict_layout(c.data(), c.size(), id0, co)) return Status::ERROR_DICTIONARY_FAILED;
  c.erase(c.begin(), c.begin() + (ptrdiff_t)co);  // (a formatted dictionary: its content)
  if (c.size() < MIN_DICT_SIZE) return Status::ERROR_INVALID_PARAMETER;
  // the samples back to back on the device (16-byte aligned starts), host samples uploaded
  size_t const n = samples.size();
  std::vector<size_t> off(n + 1, 0);
  for (size_t i = 0; i < n; i++) {
    if (!samples[i] || sample_sizes[i] == 0) return Status::ERROR_INVALID_PARAMETER;
    off[i + 1] = off[i] + ((sample_sizes[i] + 15) & ~(size_t)15);
  }
  u8 *dev = nullptr;
  if (hipMalloc(&dev, off[n] + 16) != hipSuccess) return Status::ERROR_OUT_OF_MEMORY;
  std::vector<const void *> ptrs(n);
  for (size_t i = 0; i < n && s == Status::SUCCESS; i++) {
    ptrs[i] = dev + off[i];
    s = copy_any(dev + off[i], samples[i], sample_sizes[i], stream);
  }
  std::vector<u32> counts(ZH_STATS_WORDS, 0);
  if (s == Status::SUCCESS) {
    ZstdBatchManager m(CompressionConfig::from_level(level));
    Dictionary view;
    view.raw_content = c.data();
    view.raw_size = (u32)c.size();
    s = m.set_dictionary(view);
    view.raw_content = nullptr;  // (a view: nothing to free)
    view.raw_size = 0;
    if (s == Status::SUCCESS) s = m.collect_entropy_stats(ptrs.data(), sample_sizes.data(), n, counts.data(), stream);
  }
  (void)hipFree(dev);
  if (s != Status::SUCCESS) return s;
  std::vector<u8> const fd = zh::dfin::finalize(c.data(), c.size(), counts.data(), dict_id);
  if (fd.empty() || fd.size() > MAX_DICT_SIZE) return Status::ERROR_DICTIONARY_FAILED;
  if (fd.size() > *out_size) return Status::ERROR_BUFFER_TOO_SMALL;
  memcpy(out, fd.data(), fd.size());
  *out_size = fd.size();
  return Status::SUCCESS;
}
u32 get_optimal_dict_size(size_t total) {
  size_t const s = total / 100;
  if (s < MIN_DICT_SIZE) return MIN_DICT_SIZE;
  if (s > MAX_DICT_SIZE) return MAX_DICT_SIZE;
  return (u32)((s + 1023) / 1024 * 1024);
}
bool is_valid_dictionary_size(size_t size) { return size >= MIN_DICT_SIZE && size <= MAX_DICT_SIZE; }
}  // namespace dictionary

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
std::unique_ptr<ZstdStreamingManager> create_streaming_manager(int level) {
  return std::unique_ptr<ZstdStreamingManager>(new ZstdStreamingManager(CompressionConfig::from_level(level)));
}
namespace {
// one frame through a temporary manager (level, optional dictionary), workspace allocated here
Status oneshot_compress(const void *in, size_t n, void *out, size_t *out_size, int level, const dictionary::Dictionary *dict, hipStream_t stream) {
  if (!is_valid_compression_level(level)) return Status::ERROR_INVALID_PARAMETER;
  ZstdBatchManager m(CompressionConfig::from_level(level));
  if (dict) {
    Status const sd = m.set_dictionary(*dict);
    if (sd != Status::SUCCESS) return sd;
  }
  size_t need = m.get_compress_temp_size(n);
  void *ws = nullptr;
  if (hipMalloc(&ws, need) != hipSuccess) return Status::ERROR_OUT_OF_MEMORY;
  Status s = m.compress(in, n, out, out_size, ws, need, nullptr, 0, stream);
  (void)hipFree(ws);
  return s;
}
Status oneshot_decompress(const void *in, size_t n, void *out, size_t *out_size, const dictionary::Dictionary *dict, hipStream_t stream) {
  ZstdBatchManager m;
  if (dict) {
    Status const sd = m.set_dictionary(*dict);
    if (sd != Status::SUCCESS) return sd;
  }
  size_t need = m.get_decompress_temp_size(n);
  void *ws = nullptr;
  if (hipMalloc(&ws, need) != hipSuccess) return Status::ERROR_OUT_OF_MEMORY;
  Status s = m.decompress(in, n, out, out_size, ws, need, stream);
  (void)hipFree(ws);
  return s;
}
}  // namespace
Status compress_simple(const void *in, size_t n, void *out, size_t *out_size, int level, hipStream_t stream) {
  return ZH_NOTED(oneshot_compress(in, n, out, out_size, level, nullptr, stream));
}
Status decompress_simple(const void *in, size_t n, void *out, size_t *out_size, hipStream_t stream) {
  return ZH_NOTED(oneshot_decompress(in, n, out, out_size, nullptr, stream));
}
Status compress_with_dict(const void *in, size_t n, void *out, size_t *out_size, const dictionary::Dictionary &dict, int level, hipStream_t stream) {
  return ZH_NOTED(oneshot_compress(in, n, out, out_size, level, &dict, stream));
}
Status decompress_with_dict(const void *in, size_t n, void *out, size_t *out_size, const dictionary::Dictionary &dict, hipStream_t stream) {
  return ZH_NOTED(oneshot_decompress(in, n, out, out_size, &dict, stream));
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

// Frame header fields of the first zstd frame in a buffer, after any skippable frames (the
// reference parse_zstd_frame_header skips them the same way, src/cuda_zstd_manager.cu:875-900);
// *meta_level = the level of a metadata frame written by write_metadata_frame, else -1.
namespace {
Status probe_frame(const void *data, size_t n, FrameProbe &f) {
  if (!data || n < 4) return Status::ERROR_INVALID_PARAMETER;
  size_t off = 0;
  for (int guard = 0; guard < 64; guard++) {  // (bounded number of leading skippable frames)
    u8 h[18] = {0};
    size_t const take = std::min<size_t>(n - off, sizeof(h));
    if (take < 4) return Status::ERROR_CORRUPT_DATA;
    if (copy_any(h, (const u8 *)data + off, take, 0) != Status::SUCCESS) return Status::ERROR_CUDA_ERROR;
    u32 magic;
    memcpy(&magic, h, 4);
    if ((magic & 0xFFFFFFF0u) == kSkippableMagic) {
      if (take < 8) return Status::ERROR_CORRUPT_DATA;
      u32 fs;
      memcpy(&fs, h + 4, 4);
      if (fs == 8 && take >= 16) {
        u32 cm, lv;
        memcpy(&cm, h + 8, 4);
        memcpy(&lv, h + 12, 4);
        if (cm == kMetadataMagic) f.meta_level = (int)lv;
      }
      if (n - off < 8 + (size_t)fs) return Status::ERROR_CORRUPT_DATA;
      off += 8 + (size_t)fs;
      continue;
    }
    if (magic != ZSTD_MAGIC) return Status::ERROR_INVALID_MAGIC;
    if (take < 5) return Status::ERROR_CORRUPT_DATA;
    u8 const fhd = h[4];
    u32 const fcs_flag = fhd >> 6, ss = (fhd >> 5) & 1, did = fhd & 3;
    size_t o = 5;
    if (!ss) f.window_log = 10 + (h[o++] >> 3);
    u32 const dsz = did == 0 ? 0 : did == 1 ? 1 : did == 2 ? 2 : 4;
    if (o + dsz > take) return Status::ERROR_CORRUPT_DATA;
    for (u32 k = 0; k < dsz; k++) f.dict_id |= (u32)h[o + k] << (8 * k);
    o += dsz;
    u32 const fsz = fcs_flag == 0 ? (ss ? 1 : 0) : fcs_flag == 1 ? 2 : fcs_flag == 2 ? 4 : 8;
    if (o + fsz > take) return Status::ERROR_CORRUPT_DATA;
    u64 v = 0;
    for (u32 k = 0; k < fsz; k++) v |= (u64)h[o + k] << (8 * k);
    if (fsz == 2) v += 256;
    f.content = v;
    f.has_content = fsz != 0;
    f.checksum = (fhd >> 2) & 1;
    f.frame_offset = off;
    return Status::SUCCESS;
  }
  return Status::ERROR_CORRUPT_DATA;
}
}  // namespace

Status get_decompressed_size(const void *data, size_t n, size_t *out) {
  if (!data || !out || n < 4) return Status::ERROR_INVALID_PARAMETER;
  FrameProbe f;
  Status s = probe_frame(data, n, f);
  if (s != Status::SUCCESS) return s;
  if (!f.has_content) return Status::ERROR_UNSUPPORTED_FORMAT;
  *out = (size_t)f.content;
  return Status::SUCCESS;
}
Status validate_compressed_data(const void *data, size_t n, bool) {
  FrameProbe f;
  return probe_frame(data, n, f);
}

// Skippable metadata frame (RFC 8878 §3.1.2): the reference declares SkippableFrameHeader +
// CustomMetadataFrame {custom magic, compression level} and a device writer
// (src/cuda_zstd_manager.cu:309-318, 391-412) but never calls it.  Here it is a utility: 16
// bytes [0x184D2A50][8][kMetadataMagic][level] in front of frames; every zstd decoder (libzstd,
// zh_decode.hip) skips it, extract_metadata reads the level back.
Status write_metadata_frame(void *out, size_t capacity, int level, size_t *written, hipStream_t stream) {
  if (!out || !written) return Status::ERROR_INVALID_PARAMETER;
  if (capacity < kMetadataFrameBytes) return Status::ERROR_BUFFER_TOO_SMALL;
  u32 const w[4] = {kSkippableMagic, 8u, kMetadataMagic, (u32)level};
  Status s = copy_any(out, w, sizeof(w), stream);
  if (s == Status::SUCCESS) *written = kMetadataFrameBytes;
  return s;
}

// reference is_nvcomp_zstd_format / extract_metadata (include/cuda_zstd_manager.h:415-419,
// src/cuda_zstd_manager.cu:992-1030): frame header fields after any skippable frames; the
// level comes from a metadata frame (3 when there is none, as the reference reports)
bool is_nvcomp_zstd_format(const void *data, size_t n) {
  FrameProbe f;
  return probe_frame(data, n, f) == Status::SUCCESS;
}
Status extract_metadata(const void *data, size_t n, NvcompMetadata &m) {
  FrameProbe f;
  Status s = probe_frame(data, n, f);
  if (s != Status::SUCCESS) return s;
  m.format_version = get_format_version();
  m.compression_level = f.meta_level >= 0 ? (u32)f.meta_level : 3u;
  m.uncompressed_size = f.has_content ? f.content : 0;
  m.dictionary_id = f.dict_id;
  m.checksum_policy = f.checksum ? ChecksumPolicy::COMPUTE_AND_VERIFY : ChecksumPolicy::NO_COMPUTE_NO_VERIFY;
  m.chunk_size = 128 * 1024;
  m.num_chunks = f.has_content ? (u32)((f.content + m.chunk_size - 1) / m.chunk_size) : 0;
  return Status::SUCCESS;
}

// ============================================================================
// NVCOMP v5 layer (reference src/cuda_zstd_nvcomp.cpp)
// ============================================================================
namespace nvcomp_v5 {
int status_to_nvcomp_error(Status s) {
  switch (s) {
    case Status::SUCCESS: return 0;
    case Status::ERROR_INVALID_PARAMETER: return 2;
    case Status::ERROR_OUT_OF_MEMORY: return 3;
    case Status::ERROR_CUDA_ERROR: return 4;
    case Status::ERROR_CORRUPT_DATA: return 6;
    case Status::ERROR_BUFFER_TOO_SMALL: return 7;
    case Status::ERROR_CHECKSUM_FAILED: return 10;
    case Status::ERROR_COMPRESSION: return 12;
    default: return 1;
  }
}
Status nvcomp_error_to_status(int e) {
  switch (e) {
    case 0: return Status::SUCCESS;
    case 2: return Status::ERROR_INVALID_PARAMETER;
    case 3: return Status::ERROR_OUT_OF_MEMORY;
    case 4: return Status::ERROR_CUDA_ERROR;
    case 6: return Status::ERROR_CORRUPT_DATA;
    case 7: return Status::ERROR_BUFFER_TOO_SMALL;
    case 10: return Status::ERROR_CHECKSUM_FAILED;
    case 12: return Status::ERROR_COMPRESSION;
    default: return Status::ERROR_GENERIC;
  }
}
const char *get_nvcomp_v5_error_string(int e) { return status_to_string(nvcomp_error_to_status(e)); }
bool is_nvcomp_v5_zstd_format(const void *data, size_t n) {
  if (!data || n < 4) return false;
  u32 m = 0;
  if (copy_any(&m, data, 4, 0) != Status::SUCCESS) return false;
  return m == ZSTD_MAGIC;
}
bool is_compatible_with_nvcomp_v5(u32 v) { return (v >> 16) == 5; }
NvcompV5Options to_nvcomp_v5_opts(const CompressionConfig &c) {
  NvcompV5Options o;
  o.level = c.level;
  o.chunk_size = c.block_size;
  o.enable_checksum = c.checksum != ChecksumPolicy::NO_COMPUTE_NO_VERIFY;
  return o;
}
CompressionConfig from_nvcomp_v5_opts(const NvcompV5Options &o) {
  CompressionConfig c = CompressionConfig::from_level(o.level);
  c.block_size = o.chunk_size;
  c.checksum = o.enable_checksum ? ChecksumPolicy::COMPUTE_NO_VERIFY : ChecksumPolicy::NO_COMPUTE_NO_VERIFY;
  return c;
}
std::unique_ptr<ZstdManager> create_nvcomp_v5_manager(const NvcompV5Options &o) { return create_manager(from_nvcomp_v5_opts(o)); }

class NvcompV5BatchManager::Impl {
 public:
  NvcompV5Options opts;
  ZstdBatchManager mgr;
  explicit Impl(const NvcompV5Options &o) : opts(o), mgr(config_of(o)) {}
  static CompressionConfig config_of(const NvcompV5Options &o) {  // level + checksum option
    CompressionConfig c = CompressionConfig::from_level(o.level);
    c.checksum = o.enable_checksum ? ChecksumPolicy::COMPUTE_NO_VERIFY : ChecksumPolicy::NO_COMPUTE_NO_VERIFY;
    return c;
  }
};
NvcompV5BatchManager::NvcompV5BatchManager(const NvcompV5Options &o) : pimpl_(new Impl(o)) {}
NvcompV5BatchManager::~NvcompV5BatchManager() = default;
ZstdBatchManager &NvcompV5BatchManager::batch_manager() { return pimpl_->mgr; }

template <typename T>
static Status fetch_array(std::vector<T> &dst, const T *src, size_t n, hipStream_t stream) {
  dst.resize(n);
  if (!n) return Status::SUCCESS;
  if (is_device_ptr(src)) return copy_any(dst.data(), src, n * sizeof(T), stream);
  memcpy(dst.data(), src, n * sizeof(T));
  return Status::SUCCESS;
}

size_t NvcompV5BatchManager::get_compress_temp_size(const size_t *sizes, size_t n, hipStream_t stream) const {
  if (!n || !sizes) return 0;
  std::vector<size_t> h;
  if (fetch_array(h, sizes, n, stream) != Status::SUCCESS) return 0;
  return pimpl_->mgr.get_batch_compress_temp_size(h);
}
size_t NvcompV5BatchManager::get_decompress_temp_size(const size_t *, size_t n, hipStream_t) const {
  return pimpl_->mgr.get_batch_decompress_temp_size(std::vector<size_t>(n));
}
size_t NvcompV5BatchManager::get_max_compressed_chunk_size(size_t n) const { return pimpl_->mgr.get_max_compressed_size(n); }
const CompressionStats &NvcompV5BatchManager::get_stats() const { return pimpl_->mgr.get_stats(); }

// compress_async / decompress_async: the four arrays (host or device) fetched into BatchItems, the
// batch call, and the sizes written back (0 for a failed item).  cap_of(capacity, input size) = the
// item's output capacity.
template <typename Cap, typename Call>
static Status nvcomp_batch(const void *const *d_in, const size_t *in_sizes, size_t n, void *const *d_out, size_t *out_sizes, hipStream_t stream,
                           Cap cap_of, Call call) {
  if (!n) return Status::SUCCESS;
  if (!d_in || !in_sizes || !d_out || !out_sizes) return Status::ERROR_INVALID_PARAMETER;
  std::vector<const void *> hin;
  std::vector<void *> hout;
  std::vector<size_t> hsz, hcap;
  Status s = fetch_array(hin, (const void *const *)d_in, n, stream);
  if (s == Status::SUCCESS) s = fetch_array(hout, (void *const *)d_out, n, stream);
  if (s == Status::SUCCESS) s = fetch_array(hsz, in_sizes, n, stream);
  if (s == Status::SUCCESS) s = fetch_array(hcap, (const size_t *)out_sizes, n, stream);
  if (s != Status::SUCCESS) return s;
  std::vector<BatchItem> items(n);
  for (size_t i = 0; i < n; i++) {
    items[i].input_ptr = (void *)hin[i];
    items[i].output_ptr = hout[i];
    items[i].input_size = hsz[i];
    items[i].output_size = cap_of(hcap[i], hsz[i]);
  }
  Status r = call(items);
  for (size_t i = 0; i < n; i++) hcap[i] = items[i].status == Status::SUCCESS ? items[i].output_size : 0;
  Status w = is_device_ptr(out_sizes) ? copy_any(out_sizes, hcap.data(), n * sizeof(size_t), stream) : (memcpy(out_sizes, hcap.data(), n * sizeof(size_t)), Status::SUCCESS);
  return r != Status::SUCCESS ? r : w;
}

Status NvcompV5BatchManager::compress_async(const void *const *d_in, const size_t *in_sizes, size_t n, void *const *d_out, size_t *out_sizes,
                                            void *temp, size_t temp_bytes, hipStream_t stream) {
  // reference callers pass the compressed-size array uninitialised; treat 0 as "sized with the bound"
  return nvcomp_batch(d_in, in_sizes, n, d_out, out_sizes, stream,
                      [&](size_t cap, size_t in) { return cap ? cap : get_max_compressed_chunk_size(in); },
                      [&](std::vector<BatchItem> &items) { return pimpl_->mgr.compress_batch(items, temp, temp_bytes, stream); });
}

// NvcompV5BatchManager::decompress_async (reference src/cuda_zstd_nvcomp.cpp:540-610): arrays on
// the host or the device; uncompressed_sizes in = capacity, out = bytes (0 for a failed item).
Status NvcompV5BatchManager::decompress_async(const void *const *d_in, const size_t *in_sizes, size_t n, void *const *d_out, size_t *out_sizes,
                                              void *temp, size_t temp_bytes, hipStream_t stream) {
  return nvcomp_batch(d_in, in_sizes, n, d_out, out_sizes, stream, [](size_t cap, size_t) { return cap; },
                      [&](std::vector<BatchItem> &items) { return pimpl_->mgr.decompress_batch(items, temp, temp_bytes, stream); });
}

// nvcompBatchedZstdGetDecompressSizeAsync: device arrays only, stream-ordered, nvcomp codes
Status NvcompV5BatchManager::get_decompress_sizes_async(const void *const *d_compressed_ptrs, const size_t *d_compressed_bytes,
                                                        size_t *d_uncompressed_bytes, int *d_statuses, size_t num_chunks, hipStream_t stream) {
  return pimpl_->mgr.get_decompressed_sizes_async(d_compressed_ptrs, d_compressed_bytes, num_chunks, d_uncompressed_bytes, d_statuses, stream,
                                                  true);
}

Status NvcompV5BatchManager::compress_prefix_async(const void *const *d_uncompressed_ptrs, const size_t *d_uncompressed_sizes,
                                                   const void *const *d_prefix_ptrs, const size_t *d_prefix_sizes, size_t max_chunk,
                                                   size_t num_chunks, void *const *d_compressed_ptrs, size_t *d_compressed_sizes, int *d_statuses,
                                                   void *d_temp_storage, size_t temp_storage_bytes, hipStream_t stream) {
  return pimpl_->mgr.compress_batch_device_prefix(d_uncompressed_ptrs, d_uncompressed_sizes, d_prefix_ptrs, d_prefix_sizes, max_chunk, num_chunks,
                                                  d_compressed_ptrs, d_compressed_sizes, d_statuses, d_temp_storage, temp_storage_bytes, stream);
}
Status NvcompV5BatchManager::decompress_prefix_async(const void *const *d_compressed_ptrs, const size_t *d_compressed_sizes,
                                                     const void *const *d_prefix_ptrs, const size_t *d_prefix_sizes,
                                                     const size_t *d_uncompressed_caps, size_t max_chunk, size_t num_chunks,
                                                     void *const *d_uncompressed_ptrs, size_t *d_actual_sizes, int *d_statuses,
                                                     void *d_temp_storage, size_t temp_storage_bytes, hipStream_t stream) {
  if (num_chunks && (!d_prefix_ptrs || !d_prefix_sizes)) return Status::ERROR_INVALID_PARAMETER;
  return pimpl_->mgr.decompress_batch_device_prefix(d_compressed_ptrs, d_compressed_sizes, d_prefix_ptrs, d_prefix_sizes, d_uncompressed_caps,
                                                    max_chunk, num_chunks, d_uncompressed_ptrs, d_actual_sizes, d_statuses, d_temp_storage,
                                                    temp_storage_bytes, stream);
}
Status NvcompV5BatchManager::compress_dicts_async(const void *const *d_uncompressed_ptrs, const size_t *d_uncompressed_sizes,
                                                  const int32_t *d_dict_index, size_t max_chunk, size_t num_chunks,
                                                  void *const *d_compressed_ptrs, size_t *d_compressed_sizes, int *d_statuses,
                                                  void *d_temp_storage, size_t temp_storage_bytes, hipStream_t stream) {
  return pimpl_->mgr.compress_batch_device_dicts(d_uncompressed_ptrs, d_uncompressed_sizes, d_dict_index, max_chunk, num_chunks,
                                                 d_compressed_ptrs, d_compressed_sizes, d_statuses, d_temp_storage, temp_storage_bytes, stream);
}
Status NvcompV5BatchManager::decompress_dicts_async(const void *const *d_compressed_ptrs, const size_t *d_compressed_sizes,
                                                    const int32_t *d_dict_index, const size_t *d_uncompressed_caps, size_t max_chunk,
                                                    size_t num_chunks, void *const *d_uncompressed_ptrs, size_t *d_actual_sizes,
                                                    int *d_statuses, void *d_temp_storage, size_t temp_storage_bytes, hipStream_t stream) {
  return pimpl_->mgr.decompress_batch_device_dicts(d_compressed_ptrs, d_compressed_sizes, d_dict_index, d_uncompressed_caps, max_chunk,
                                                   num_chunks, d_uncompressed_ptrs, d_actual_sizes, d_statuses, d_temp_storage,
                                                   temp_storage_bytes, stream);
}

Status get_metadata_async(const void *d, size_t n, NvcompV5Metadata *m, hipStream_t) {
  if (!m) return Status::ERROR_INVALID_PARAMETER;
  size_t s;
  Status st = get_decompressed_size(d, n, &s);
  if (st != Status::SUCCESS) return st;
  m->uncompressed_size = s;
  m->compressed_size = n;
  m->num_chunks = 1;
  m->chunk_size = (u32)std::min<size_t>(s, 0xFFFFFFFFu);
  return Status::SUCCESS;
}
Status get_metadata(const void *d, size_t n, NvcompV5Metadata &m) { return get_metadata_async(d, n, &m, 0); }
bool validate_metadata(const NvcompV5Metadata &m) { return is_compatible_with_nvcomp_v5(m.format_version); }
Status get_decompressed_size_async(const void *d, size_t n, size_t *out, hipStream_t) { return get_decompressed_size(d, n, out); }
Status get_num_chunks(const void *d, size_t n, size_t *out) {
  size_t s;
  Status st = get_decompressed_size(d, n, &s);
  if (st == Status::SUCCESS && out) *out = 1;
  return st;
}
Status get_chunk_sizes(const void *d, size_t n, size_t *sizes, size_t max_chunks) {
  if (!sizes || !max_chunks) return Status::ERROR_INVALID_PARAMETER;
  return get_decompressed_size(d, n, sizes);
}
}  // namespace nvcomp_v5

// ============================================================================
// HybridEngine (reference src/cuda_zstd_hybrid.cu)
// ============================================================================
// Throughput history for ADAPTIVE routing (reference src/cuda_zstd_hybrid.cu:46-136): a
// 64-sample ring per (CPU | GPU, compress | decompress), MB/s = MiB of input (compress) or of
// output (decompress) per second of the call.
struct ThroughputHistory {
  static constexpr size_t kMax = 64;
  double ring[4][kMax] = {};
  size_t count[4] = {};
  static size_t slot(ExecutionBackend b, bool comp) {
    bool const cpu = b == ExecutionBackend::CPU_LIBZSTD || b == ExecutionBackend::CPU_PARALLEL;
    return (cpu ? 0u : 2u) + (comp ? 0u : 1u);
  }
  void record(ExecutionBackend b, bool comp, double mbps) {
    size_t const k = slot(b, comp);
    ring[k][count[k] % kMax] = mbps;
    count[k]++;
  }
  double average(ExecutionBackend b, bool comp) const {
    size_t const k = slot(b, comp), n = std::min(count[k], kMax);
    if (!n) return 0.0;
    double s = 0;
    for (size_t i = 0; i < n; i++) s += ring[k][i];
    return s / (double)n;
  }
  void reset() { for (size_t &c : count) c = 0; }
};

class HybridEngine::Impl {
 public:
  HybridConfig config;
  CompressionStats stats;
  ThroughputHistory prof;
  mutable std::mutex mu;  // guards prof (get_observed_throughput may run beside a call)
  ZstdBatchManager mgr;
  explicit Impl(const HybridConfig &c) : config(c), mgr(CompressionConfig::from_level(c.compression_level)) {}
  void profile(ExecutionBackend b, bool comp, size_t bytes, double ms) {
    if (!config.enable_profiling) return;
    std::lock_guard<std::mutex> g(mu);
    prof.record(b, comp, ms > 0 ? ((double)bytes / (1024.0 * 1024.0)) / (ms / 1000.0) : 0.0);
  }
};
HybridEngine::HybridEngine() : pimpl_(new Impl(HybridConfig{})) {}
HybridEngine::HybridEngine(const HybridConfig &c) : pimpl_(new Impl(c)) {}
HybridEngine::~HybridEngine() = default;
HybridEngine::HybridEngine(HybridEngine &&) noexcept = default;
HybridEngine &HybridEngine::operator=(HybridEngine &&) noexcept = default;
double HybridEngine::get_observed_throughput(ExecutionBackend b, bool comp) const {
  std::lock_guard<std::mutex> g(pimpl_->mu);
  return pimpl_->prof.average(b, comp);
}
void HybridEngine::reset_profiling() {
  std::lock_guard<std::mutex> g(pimpl_->mu);
  pimpl_->prof.reset();
}
Status HybridEngine::configure(const HybridConfig &c) {
  if (!is_valid_compression_level(c.compression_level)) return Status::ERROR_INVALID_PARAMETER;
  pimpl_->config = c;
  return pimpl_->mgr.set_compression_level(c.compression_level);
}
HybridConfig HybridEngine::get_config() const { return pimpl_->config; }
Status HybridEngine::set_compression_level(int level) {
  if (!is_valid_compression_level(level)) return Status::ERROR_INVALID_PARAMETER;
  pimpl_->config.compression_level = level;
  return pimpl_->mgr.set_compression_level(level);
}
DataLocation HybridEngine::detect_location(const void *p) { return is_device_ptr(p) ? DataLocation::DEVICE : DataLocation::HOST; }
ExecutionBackend HybridEngine::query_routing(size_t n, DataLocation il, DataLocation ol, bool is_compression) const {
  HybridMode m = pimpl_->config.mode;
  if (m == HybridMode::FORCE_CPU) return ExecutionBackend::CPU_LIBZSTD;
  if (m == HybridMode::FORCE_GPU) return ExecutionBackend::GPU_KERNELS;
  bool const dev = il == DataLocation::DEVICE && ol == DataLocation::DEVICE;
  if (m == HybridMode::PREFER_GPU) return (il == DataLocation::HOST && ol == DataLocation::HOST) ? ExecutionBackend::CPU_LIBZSTD : ExecutionBackend::GPU_KERNELS;
  if (m == HybridMode::PREFER_CPU) return dev ? ExecutionBackend::GPU_KERNELS : ExecutionBackend::CPU_LIBZSTD;
  if (m == HybridMode::ADAPTIVE) {
    // reference src/cuda_zstd_hybrid.cu:215-240: with samples of both, the GPU when > 1.2x the CPU
    double const cpu = get_observed_throughput(ExecutionBackend::CPU_LIBZSTD, is_compression);
    double const gpu = get_observed_throughput(ExecutionBackend::GPU_KERNELS, is_compression);
    if (cpu > 0.0 && gpu > 0.0) return gpu > 1.2 * cpu ? ExecutionBackend::GPU_KERNELS : ExecutionBackend::CPU_LIBZSTD;
  }
  // AUTO (and ADAPTIVE without history): device-resident data stays on the device; host data
  // goes to libzstd
  (void)n;
  return dev ? ExecutionBackend::GPU_KERNELS : ExecutionBackend::CPU_LIBZSTD;
}
size_t HybridEngine::get_max_compressed_size(size_t n) const {
  LibZstd &z = libzstd();
  size_t a = estimate_compressed_size(n, pimpl_->config.compression_level);
  return z.ok ? std::max(a, z.compressBound(n)) : a;
}
CompressionStats HybridEngine::get_stats() const { return pimpl_->stats; }
void HybridEngine::reset_stats() { pimpl_->stats = CompressionStats{}; }

Status HybridEngine::compress(const void *in, size_t n, void *out, size_t *out_size, DataLocation il, DataLocation ol, HybridResult *res,
                              hipStream_t stream) {
  if (!in || !out || !out_size || n == 0) return Status::ERROR_INVALID_PARAMETER;
  if (il == DataLocation::UNKNOWN) il = detect_location(in);
  if (ol == DataLocation::UNKNOWN) ol = detect_location(out);
  auto t0 = std::chrono::steady_clock::now();
  ExecutionBackend be = query_routing(n, il, ol, true);
  Status s;
  if (be == ExecutionBackend::CPU_LIBZSTD) {
    s = cpu_compress(in, n, out, out_size, pimpl_->config.compression_level, stream);
  } else {
    // device pipeline: stage host buffers through device memory when needed
    const void *din = in;
    void *dout = out, *tmp_in = nullptr, *tmp_out = nullptr, *ws = nullptr;
    size_t const cap = *out_size;
    s = Status::SUCCESS;
    if (il != DataLocation::DEVICE) {
      if (hipMalloc(&tmp_in, n) != hipSuccess) s = Status::ERROR_OUT_OF_MEMORY;
      else s = copy_any(tmp_in, in, n, stream);
      din = tmp_in;
    }
    if (s == Status::SUCCESS && ol != DataLocation::DEVICE) {
      if (hipMalloc(&tmp_out, cap) != hipSuccess) s = Status::ERROR_OUT_OF_MEMORY;
      dout = tmp_out;
    }
    size_t need = pimpl_->mgr.get_compress_temp_size(n);
    if (s == Status::SUCCESS && hipMalloc(&ws, need) != hipSuccess) s = Status::ERROR_OUT_OF_MEMORY;
    if (s == Status::SUCCESS) s = pimpl_->mgr.compress(din, n, dout, out_size, ws, need, nullptr, 0, stream);
    if (s == Status::SUCCESS && tmp_out) s = copy_any(out, tmp_out, *out_size, stream);
    if (tmp_in) (void)hipFree(tmp_in);
    if (tmp_out) (void)hipFree(tmp_out);
    if (ws) (void)hipFree(ws);
  }
  double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (s == Status::SUCCESS) {
    pimpl_->stats.input_bytes += n;
    pimpl_->stats.output_bytes += *out_size;
    pimpl_->stats.compression_time_ms += ms;
    pimpl_->profile(be, true, n, ms);
  }
  if (res) {
    res->backend_used = be;
    res->input_location = il;
    res->output_location = ol;
    res->total_time_ms = ms;
    res->compute_time_ms = ms;
    res->input_bytes = n;
    res->output_bytes = s == Status::SUCCESS ? *out_size : 0;
    res->compression_ratio = (s == Status::SUCCESS && *out_size) ? (float)n / *out_size : 0.f;
    res->throughput_mbps = ms > 0 ? n / 1e6 / (ms / 1e3) : 0;
    res->routing_reason = be == ExecutionBackend::CPU_LIBZSTD ? "cpu (libzstd)" : "gpu (gfx950 kernels)";
  }
  return ZH_NOTED(s);
}

// same routing as compress (reference src/cuda_zstd_hybrid.cu:836-905): libzstd for host data /
// FORCE_CPU, the gfx950 decoder for device data (host buffers staged through HBM when forced)
Status HybridEngine::decompress(const void *in, size_t n, void *out, size_t *out_size, DataLocation il, DataLocation ol, HybridResult *res,
                                hipStream_t stream) {
  if (!in || !out || !out_size || n < 4) return Status::ERROR_INVALID_PARAMETER;
  if (il == DataLocation::UNKNOWN) il = detect_location(in);
  if (ol == DataLocation::UNKNOWN) ol = detect_location(out);
  auto t0 = std::chrono::steady_clock::now();
  ExecutionBackend be = query_routing(n, il, ol, false);
  Status s;
  if (be == ExecutionBackend::CPU_LIBZSTD) {
    s = cpu_decompress(in, n, out, out_size, stream);
  } else {
    const void *din = in;
    void *dout = out, *tmp_in = nullptr, *tmp_out = nullptr, *ws = nullptr;
    size_t const cap = *out_size;
    s = Status::SUCCESS;
    if (il != DataLocation::DEVICE) {
      if (hipMalloc(&tmp_in, n) != hipSuccess) s = Status::ERROR_OUT_OF_MEMORY;
      else s = copy_any(tmp_in, in, n, stream);
      din = tmp_in;
    }
    if (s == Status::SUCCESS && ol != DataLocation::DEVICE) {
      if (hipMalloc(&tmp_out, std::max<size_t>(cap, 1)) != hipSuccess) s = Status::ERROR_OUT_OF_MEMORY;
      dout = tmp_out;
    }
    size_t need = pimpl_->mgr.get_decompress_temp_size(n);
    if (s == Status::SUCCESS && hipMalloc(&ws, need) != hipSuccess) s = Status::ERROR_OUT_OF_MEMORY;
    if (s == Status::SUCCESS) s = pimpl_->mgr.decompress(din, n, dout, out_size, ws, need, stream);
    if (s == Status::SUCCESS && tmp_out) s = copy_any(out, tmp_out, *out_size, stream);
    if (tmp_in) (void)hipFree(tmp_in);
    if (tmp_out) (void)hipFree(tmp_out);
    if (ws) (void)hipFree(ws);
  }
  double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (s == Status::SUCCESS) {
    pimpl_->stats.bytes_decompressed += *out_size;
    pimpl_->stats.decompression_time_ms += ms;
    pimpl_->profile(be, false, *out_size, ms);
  }
  if (res) {
    res->backend_used = be;
    res->input_location = il;
    res->output_location = ol;
    res->total_time_ms = ms;
    res->compute_time_ms = ms;
    res->input_bytes = n;
    res->output_bytes = s == Status::SUCCESS ? *out_size : 0;
  }
  return ZH_NOTED(s);
}

// reference src/cuda_zstd_hybrid.cu:912-992: items one by one through the routing; per-item
// BatchRoutingResult; ERROR_COMPRESSION / ERROR_DECOMPRESSION when any item failed
Status HybridEngine::compress_batch(const void *const *inputs, const size_t *sizes, void **outputs, size_t *out_sizes, size_t count,
                                    DataLocation il, DataLocation ol, BatchRoutingResult *results, hipStream_t stream) {
  if (!inputs || !sizes || !outputs || !out_sizes || count == 0) return ZH_NOTED(Status::ERROR_INVALID_PARAMETER);
  bool ok = true;
  for (size_t i = 0; i < count; i++) {
    HybridResult r;
    Status s = compress(inputs[i], sizes[i], outputs[i], &out_sizes[i], il, ol, &r, stream);
    if (results) {
      results[i].item_index = i;
      results[i].backend_used = r.backend_used;
      results[i].status = s;
      results[i].input_bytes = sizes[i];
      results[i].output_bytes = out_sizes[i];
      results[i].compute_time_ms = r.compute_time_ms;
    }
    ok &= s == Status::SUCCESS;
  }
  return ok ? Status::SUCCESS : ZH_NOTED(Status::ERROR_COMPRESSION);
}
Status HybridEngine::decompress_batch(const void *const *inputs, const size_t *sizes, void **outputs, size_t *out_sizes, size_t count,
                                      DataLocation il, DataLocation ol, BatchRoutingResult *results, hipStream_t stream) {
  if (!inputs || !sizes || !outputs || !out_sizes || count == 0) return ZH_NOTED(Status::ERROR_INVALID_PARAMETER);
  bool ok = true;
  for (size_t i = 0; i < count; i++) {
    HybridResult r;
    Status s = decompress(inputs[i], sizes[i], outputs[i], &out_sizes[i], il, ol, &r, stream);
    if (results) {
      results[i].item_index = i;
      results[i].backend_used = r.backend_used;
      results[i].status = s;
      results[i].input_bytes = sizes[i];
      results[i].output_bytes = out_sizes[i];
      results[i].compute_time_ms = r.compute_time_ms;
    }
    ok &= s == Status::SUCCESS;
  }
  return ok ? Status::SUCCESS : ZH_NOTED(Status::ERROR_DECOMPRESSION);
}

Status hybrid_decompress(const void *in, size_t n, void *out, size_t *out_size, DataLocation il, DataLocation ol, HybridResult *res, hipStream_t stream) {
  HybridEngine e;
  return e.decompress(in, n, out, out_size, il, ol, res, stream);
}
Status hybrid_compress(const void *in, size_t n, void *out, size_t *out_size, DataLocation il, DataLocation ol, int level, HybridResult *res,
                       hipStream_t stream) {
  HybridConfig c;
  c.compression_level = level;
  HybridEngine e(c);
  return e.compress(in, n, out, out_size, il, ol, res, stream);
}
std::unique_ptr<HybridEngine> create_hybrid_engine(const HybridConfig &c) { return std::unique_ptr<HybridEngine>(new HybridEngine(c)); }
std::unique_ptr<HybridEngine> create_hybrid_engine(int level) {
  HybridConfig c;
  c.compression_level = level;
  return create_hybrid_engine(c);
}

// ============================================================================
// adaptive level selection (include/cuda_zstd_adaptive.h; reference src/cuda_zstd_adaptive.cu)
// ============================================================================
namespace {
// One device buffer through the batch kernels (zh_adaptive.hip): the record, the statistics and
// the level live in one small allocation; one copy back, one wait.
Status adaptive_one(const void *d_data, size_t size, size_t sample_bytes, int preference, cuda_zstd_adaptive_stats_t &out, hipStream_t stream) {
  if (!d_data || size == 0 || sample_bytes == 0 || preference < 0 || preference > 2) return Status::ERROR_INVALID_PARAMETER;
  size_t const rec = ZH_AD_REC_WORDS * sizeof(u32);
  u8 *d = nullptr;
  if (hipMalloc((void **)&d, rec + sizeof(out) + sizeof(int)) != hipSuccess) { (void)hipGetLastError(); return Status::ERROR_OUT_OF_MEMORY; }
  auto *const d_stats = (cuda_zstd_adaptive_stats_t *)(d + rec);
  bool const ok = zh::adaptive_launch(nullptr, nullptr, d_data, size, 1, std::min(sample_bytes, size), preference, d_stats,
                                      (int *)(d + rec + sizeof(out)), (u32 *)d, stream) == hipSuccess &&
                  hipMemcpyAsync(&out, d_stats, sizeof(out), hipMemcpyDeviceToHost, stream) == hipSuccess &&
                  hipStreamSynchronize(stream) == hipSuccess;
  (void)hipFree(d);
  if (!ok) { (void)hipGetLastError(); return Status::ERROR_CUDA_ERROR; }
  return Status::SUCCESS;
}

// The branch of the rule behind a result (the level table's rows differ, except RANDOM / LOW)
int adaptive_branch(const cuda_zstd_adaptive_stats_t &s, int preference) {
  if (!s.sample_size) return ZH_AD_EMPTY;
  if (s.flags & ZH_AD_IS_RANDOM) return ZH_AD_RANDOM;
  for (int b = ZH_AD_REPETITIVE; b < ZH_AD_LOW; b++)
    if (zh_adaptive_level(b, preference) == s.level) return b;
  return ZH_AD_LOW;
}
const char *const kAdaptiveReasoning[ZH_AD_BRANCHES] = {
    "high entropy and no short-period patterns: the data looks random, a fast level loses nothing",
    "long runs or mostly repeated bytes: a deep search is cheap here and pays",
    "low entropy with many repeated bytes: highly compressible, a strong level pays",
    "moderately compressible: a middle level",
    "little redundancy in the byte statistics: a fast level",
    "empty input: the default level",
};
}  // namespace

namespace adaptive {

AdaptiveLevelSelector::AdaptiveLevelSelector() = default;
AdaptiveLevelSelector::AdaptiveLevelSelector(AdaptivePreference pref) : preference_(pref) {}
AdaptiveLevelSelector::~AdaptiveLevelSelector() = default;
void AdaptiveLevelSelector::set_preference(AdaptivePreference pref) { preference_ = pref; }
void AdaptiveLevelSelector::set_sample_size(size_t size) { sample_size_ = size; }
void AdaptiveLevelSelector::enable_quick_analysis(bool enable) { quick_mode_ = enable; }  // (never read: see the header)
const DataCharacteristics &AdaptiveLevelSelector::get_last_characteristics() const { return last_characteristics_; }
void AdaptiveLevelSelector::reset_statistics() { last_characteristics_ = DataCharacteristics(); }

Status AdaptiveLevelSelector::select_level(const void *d_data, size_t data_size, AdaptiveResult &result, hipStream_t stream) {
  cuda_zstd_adaptive_stats_t s;
  Status const st = adaptive_one(d_data, data_size, sample_size_, (int)preference_, s, stream);
  if (st != Status::SUCCESS) return ZH_NOTED(st);
  DataCharacteristics &c = last_characteristics_;
  c.entropy = s.entropy;
  c.repetition_ratio = s.repetition_ratio;
  c.compressibility = s.compressibility;
  c.unique_bytes = s.unique_bytes;
  c.max_run_length = s.max_run_length;
  c.avg_match_length = 0;
  c.has_patterns = (s.flags & ZH_AD_HAS_PATTERNS) != 0;
  c.is_random = (s.flags & ZH_AD_IS_RANDOM) != 0;
  result.recommended_level = s.level;
  result.recommended_strategy = CompressionConfig::level_to_strategy(s.level);
  result.characteristics = c;
  result.confidence = 0.85f;
  result.reasoning = kAdaptiveReasoning[adaptive_branch(s, (int)preference_)];
  return Status::SUCCESS;
}

Status select_adaptive_level(const void *d_data, size_t data_size, int &recommended_level, AdaptivePreference preference, hipStream_t stream) {
  AdaptiveResult r;
  Status const st = AdaptiveLevelSelector(preference).select_level(d_data, data_size, r, stream);
  if (st == Status::SUCCESS) recommended_level = r.recommended_level;
  return st;
}
Status analyze_and_select(const void *d_data, size_t data_size, AdaptiveResult &result, AdaptivePreference preference, hipStream_t stream) {
  return AdaptiveLevelSelector(preference).select_level(d_data, data_size, result, stream);
}
Status is_compressible(const void *d_data, size_t data_size, bool &compressible, float &estimated_ratio, hipStream_t stream) {
  AdaptiveResult r;
  Status const st = AdaptiveLevelSelector(AdaptivePreference::BALANCED).select_level(d_data, data_size, r, stream);
  if (st != Status::SUCCESS) return st;
  compressible = r.characteristics.compressibility > 0.3f;
  estimated_ratio = 1.0f + r.characteristics.compressibility * 3.0f;
  return Status::SUCCESS;
}

}  // namespace adaptive

}  // namespace cuda_zstd

// ============================================================================
// C ABI (reference src/cuda_zstd_c_api.cpp:10-209, src/cuda_zstd_nvcomp.cpp:766-840)
// ============================================================================
using namespace cuda_zstd;
using nvcomp_v5::status_to_nvcomp_error;

struct cuda_zstd_manager_t { std::unique_ptr<ZstdBatchManager> manager; };
// the handle owns the bytes; `dict` is the reference-shaped view of them (its copy operations
// would malloc, so it is never copied here)
struct cuda_zstd_dict_t {
  std::vector<u8> bytes;
  std::unique_ptr<dictionary::Dictionary> dict;
  void set(std::vector<u8> &&b, u32 id) {
    bytes = std::move(b);
    dict.reset(new dictionary::Dictionary);
    dict->raw_content = bytes.data();
    dict->raw_size = (u32)bytes.size();
    dict->header.dictionary_id = id;
    dict->header.raw_content_size = (u32)bytes.size();
  }
};
struct cuda_zstd_dict_set_t { std::unique_ptr<DictionarySet> set; };
struct nvcomp_zstd_batch_manager_t { std::unique_ptr<nvcomp_v5::NvcompV5BatchManager> mgr; };
struct cuda_zstd_hybrid_engine_t { std::unique_ptr<HybridEngine> engine; };

// every C entry's Status -> the reference's int codes; failures also go to the last-error slot
static int c_err(Status s) { return status_to_nvcomp_error(s == Status::SUCCESS ? s : noted(s, "C API", 0)); }

extern "C" {

cuda_zstd_manager_t *cuda_zstd_create_manager(int level) {
  try {
    if (!is_valid_compression_level(level)) return nullptr;
    auto *m = new cuda_zstd_manager_t;
    m->manager.reset(new ZstdBatchManager(CompressionConfig::from_level(level)));
    return m;
  } catch (...) {
    return nullptr;
  }
}
void cuda_zstd_destroy_manager(cuda_zstd_manager_t *m) { delete m; }

int cuda_zstd_compress(cuda_zstd_manager_t *m, const void *src, size_t n, void *dst, size_t *dst_size, void *ws, size_t ws_size, hipStream_t stream) {
  if (!m || !m->manager) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(m->manager->compress(src, n, dst, dst_size, ws, ws_size, nullptr, 0, stream));
}
int cuda_zstd_decompress(cuda_zstd_manager_t *m, const void *src, size_t n, void *dst, size_t *dst_size, void *ws, size_t ws_size, hipStream_t stream) {
  if (!m || !m->manager) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(m->manager->decompress(src, n, dst, dst_size, ws, ws_size, stream));
}
size_t cuda_zstd_get_compress_workspace_size(cuda_zstd_manager_t *m, size_t n) { return (m && m->manager) ? m->manager->get_compress_temp_size(n) : 0; }
size_t cuda_zstd_get_decompress_workspace_size(cuda_zstd_manager_t *m, size_t n) { return (m && m->manager) ? m->manager->get_decompress_temp_size(n) : 0; }
size_t cuda_zstd_get_max_compressed_size(cuda_zstd_manager_t *m, size_t n) { return (m && m->manager) ? m->manager->get_max_compressed_size(n) : 0; }

cuda_zstd_dict_t *cuda_zstd_train_dictionary_params(const void **samples, const size_t *sizes, size_t num, size_t dict_size, unsigned k,
                                                    unsigned d) {
  if (!samples || !sizes || num == 0 || dict_size == 0) return nullptr;
  try {
    // COVER-trained raw content (zh_dict.cpp), replacing the reference's n-gram fill
    // (src/cuda_zstd_dictionary.cu:179-415); samples are host buffers
    std::vector<std::pair<const u8 *, size_t>> s;
    for (size_t i = 0; i < num; i++) {
      if (!samples[i] || sizes[i] == 0) return nullptr;  // (reference src/cuda_zstd_c_api.cpp:142-145)
      s.emplace_back((const u8 *)samples[i], sizes[i]);
    }
    std::vector<u8> c = zh::cover_train(s, std::min(dict_size, zh::kDictMaxBytes), k ? k : zh::kCoverDefaultK, d ? d : zh::kCoverDefaultD);
    if (c.size() < dictionary::MIN_DICT_SIZE) return nullptr;  // (set_dictionary would refuse it)
    auto *h = new cuda_zstd_dict_t;
    h->set(std::move(c), 0);
    return h;
  } catch (...) {
    return nullptr;
  }
}
cuda_zstd_dict_t *cuda_zstd_train_dictionary(const void **samples, const size_t *sizes, size_t num, size_t dict_size) {
  return cuda_zstd_train_dictionary_params(samples, sizes, num, dict_size, 0, 0);
}
size_t cuda_zstd_train_dictionary_device_get_temp_size(size_t total_sample_bytes, size_t num_samples, size_t dict_size, unsigned k) {
  return zh::cover_temp_bytes(total_sample_bytes, num_samples, dict_size, k);
}
int cuda_zstd_train_dictionary_device(const void *d_samples, const size_t *sizes, size_t num, size_t dict_size, unsigned k, unsigned d,
                                      void *d_temp, size_t temp_bytes, hipStream_t stream, cuda_zstd_dict_t **dict_out) {
  if (!dict_out) return c_err(Status::ERROR_INVALID_PARAMETER);
  *dict_out = nullptr;
  if (!d_samples || !sizes || num == 0 || !dictionary::is_valid_dictionary_size(dict_size)) return c_err(Status::ERROR_INVALID_PARAMETER);
  try {
    std::vector<u8> c;
    Status const st = dictionary::train_device((const u8 *)d_samples, sizes, num, dict_size, k, d, d_temp, temp_bytes, false, stream, c);
    if (st != Status::SUCCESS) return c_err(st);
    if (c.size() < dictionary::MIN_DICT_SIZE) return c_err(Status::ERROR_COMPRESSION);  // (where the host entry returns NULL)
    auto *h = new cuda_zstd_dict_t;
    h->set(std::move(c), 0);
    *dict_out = h;
    return 0;
  } catch (...) {
    return c_err(Status::ERROR_OUT_OF_MEMORY);
  }
}
size_t cuda_zstd_train_dictionaries_device_get_temp_size(const size_t *sizes, size_t num, const size_t *counts, size_t num_groups, size_t dict_size,
                                                         unsigned k) {
  if (!sizes || !counts || num_groups == 0 || num_groups > zh::kCoverMaxGroups) return 0;
  size_t counted = 0;
  for (size_t g = 0; g < num_groups; g++) {
    if (counts[g] > num - counted) return 0;
    counted += counts[g];
  }
  return counted == num ? zh::cover_temp_bytes(sizes, num, counts, num_groups, dict_size, k) : 0;
}
int cuda_zstd_train_dictionaries_device(const void *d_samples, const size_t *sizes, size_t num, const size_t *counts, size_t num_groups,
                                        size_t dict_size, unsigned k, unsigned d, void *d_temp, size_t temp_bytes, hipStream_t stream,
                                        cuda_zstd_dict_t **dicts_out, int *group_status) {
  if (!dicts_out || num_groups == 0 || num_groups > zh::kCoverMaxGroups) return c_err(Status::ERROR_INVALID_PARAMETER);
  for (size_t g = 0; g < num_groups; g++) dicts_out[g] = nullptr;
  if (group_status)
    for (size_t g = 0; g < num_groups; g++) group_status[g] = status_to_nvcomp_error(Status::ERROR_COMPRESSION);
  if (!d_samples || !sizes || !counts || num == 0 || !dictionary::is_valid_dictionary_size(dict_size)) return c_err(Status::ERROR_INVALID_PARAMETER);
  try {
    std::vector<std::vector<u8>> c;
    Status const st =
        dictionary::train_groups_device((const u8 *)d_samples, sizes, num, counts, num_groups, dict_size, k, d, d_temp, temp_bytes, false, stream, c);
    if (st != Status::SUCCESS) return c_err(st);
    for (size_t g = 0; g < num_groups; g++) {
      if (c[g].size() < dictionary::MIN_DICT_SIZE) continue;  // (where the host entry returns NULL): the group's status stays 12
      auto *h = new cuda_zstd_dict_t;
      h->set(std::move(c[g]), 0);
      dicts_out[g] = h;
      if (group_status) group_status[g] = 0;
    }
    return 0;
  } catch (...) {
    for (size_t g = 0; g < num_groups; g++) {
      delete dicts_out[g];
      dicts_out[g] = nullptr;
    }
    return c_err(Status::ERROR_OUT_OF_MEMORY);
  }
}
// on != 0: later device trainings time their kernel groups with HIP events; ms3 (optional): the
// last such call's ids + freq, prevdist and step-loop milliseconds
void cuda_zstd_hip_dict_train_profile(int on, double *ms3) {
  dictionary::g_train_profile = on != 0;
  if (ms3)
    for (int i = 0; i < 3; i++) ms3[i] = dictionary::g_train_phase_ms[i];
}
int cuda_zstd_finalize_dictionary(const cuda_zstd_dict_t *content, const void *const *samples, const size_t *sizes, size_t num, int level,
                                  unsigned dict_id, hipStream_t stream, cuda_zstd_dict_t **dict_out) {
  if (!dict_out) return c_err(Status::ERROR_INVALID_PARAMETER);
  *dict_out = nullptr;
  if (!content || !content->dict || !samples || !sizes || num == 0) return c_err(Status::ERROR_INVALID_PARAMETER);
  try {
    std::vector<u8> out(content->bytes.size() + 512);
    size_t n = out.size();
    Status const st = dictionary::finalize_dictionary(content->bytes.data(), content->bytes.size(), std::vector<const void *>(samples, samples + num),
                                                      std::vector<size_t>(sizes, sizes + num), level, dict_id, out.data(), &n, stream);
    if (st != Status::SUCCESS) return c_err(st);
    out.resize(n);
    u32 id = 0;
    memcpy(&id, out.data() + 4, 4);
    auto *h = new cuda_zstd_dict_t;
    h->set(std::move(out), id);
    *dict_out = h;
    return 0;
  } catch (...) {
    return c_err(Status::ERROR_OUT_OF_MEMORY);
  }
}
void cuda_zstd_destroy_dictionary(cuda_zstd_dict_t *d) { delete d; }
// reference DictionaryManager::load_dictionary (include/cuda_zstd_dictionary.h:292-310): a host
// buffer with raw content or a formatted dictionary (e.g. ZDICT_trainFromBuffer's)
cuda_zstd_dict_t *cuda_zstd_load_dictionary(const void *buffer, size_t size) {
  // the managers' set_dictionary limits (MIN_DICT_SIZE .. MAX_DICT_SIZE, reference
  // src/cuda_zstd_manager.cu:3711-3736) apply here already, so a handle is always settable
  if (!buffer || size < dictionary::MIN_DICT_SIZE || size > zh::kDictMaxBytes) return nullptr;
  u32 id = 0;
  size_t off = 0;
  if (!zh::dict_layout((const u8 *)buffer, size, id, off)) return nullptr;
  try {
    auto *d = new cuda_zstd_dict_t;
    d->set(std::vector<u8>((const u8 *)buffer, (const u8 *)buffer + size), id);
    return d;
  } catch (...) {
    return nullptr;
  }
}
size_t cuda_zstd_get_dictionary_content(const cuda_zstd_dict_t *d, void *out, size_t capacity) {
  if (!d || !d->dict) return 0;
  size_t const n = d->bytes.size();
  if (out && capacity >= n) memcpy(out, d->bytes.data(), n);
  return n;
}
int cuda_zstd_get_dictionary_layout(const cuda_zstd_dict_t *d, unsigned int *dict_id, size_t *content_offset) {
  if (!d || !d->dict) return c_err(Status::ERROR_INVALID_PARAMETER);
  u32 id = 0;
  size_t off = 0;
  if (!zh::dict_layout(d->bytes.data(), d->bytes.size(), id, off)) return c_err(Status::ERROR_DICTIONARY_FAILED);
  if (dict_id) *dict_id = id;
  if (content_offset) *content_offset = off;
  return 0;
}
int cuda_zstd_clear_dictionary(cuda_zstd_manager_t *m) {
  if (!m || !m->manager) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(m->manager->clear_dictionary());
}
int cuda_zstd_set_dictionary(cuda_zstd_manager_t *m, cuda_zstd_dict_t *d) {
  if (!m || !m->manager || !d || !d->dict) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(m->manager->set_dictionary(*d->dict));
}
const char *cuda_zstd_get_error_string(int code) { return status_to_string(nvcomp_v5::nvcomp_error_to_status(code)); }
int cuda_zstd_is_error(int code) { return code != 0; }

size_t cuda_zstd_get_batch_compress_workspace_size(cuda_zstd_manager_t *m, const size_t *sizes, size_t count) {
  if (!m || !m->manager || (!sizes && count)) return 0;
  return m->manager->get_batch_compress_temp_size(std::vector<size_t>(sizes, sizes + count));
}
int cuda_zstd_compress_batch(cuda_zstd_manager_t *m, const void *const *in_ptrs, const size_t *in_sizes, size_t count, void *const *out_ptrs,
                             size_t *out_sizes, int *statuses, void *ws, size_t ws_size, hipStream_t stream) {
  if (!m || !m->manager || (count && (!in_ptrs || !in_sizes || !out_ptrs || !out_sizes))) return c_err(Status::ERROR_INVALID_PARAMETER);
  std::vector<BatchItem> items(count);
  for (size_t i = 0; i < count; i++) {
    items[i].input_ptr = (void *)in_ptrs[i];
    items[i].output_ptr = out_ptrs[i];
    items[i].input_size = in_sizes[i];
    items[i].output_size = out_sizes[i];
  }
  Status s = m->manager->compress_batch(items, ws, ws_size, stream);
  for (size_t i = 0; i < count; i++) {
    if (items[i].status == Status::SUCCESS) out_sizes[i] = items[i].output_size;
    if (statuses) statuses[i] = c_err(items[i].status);
  }
  return c_err(s);
}
size_t cuda_zstd_get_batch_decompress_workspace_size(cuda_zstd_manager_t *m, const size_t *sizes, size_t count) {
  if (!m || !m->manager || (!sizes && count)) return 0;
  return m->manager->get_batch_decompress_temp_size(std::vector<size_t>(sizes, sizes + count));
}
int cuda_zstd_decompress_batch(cuda_zstd_manager_t *m, const void *const *in_ptrs, const size_t *in_sizes, size_t count, void *const *out_ptrs,
                               size_t *out_sizes, int *statuses, void *ws, size_t ws_size, hipStream_t stream) {
  if (!m || !m->manager || (count && (!in_ptrs || !in_sizes || !out_ptrs || !out_sizes))) return c_err(Status::ERROR_INVALID_PARAMETER);
  std::vector<BatchItem> items(count);
  for (size_t i = 0; i < count; i++) {
    items[i].input_ptr = (void *)in_ptrs[i];
    items[i].output_ptr = out_ptrs[i];
    items[i].input_size = in_sizes[i];
    items[i].output_size = out_sizes[i];
  }
  Status s = m->manager->decompress_batch(items, ws, ws_size, stream);
  for (size_t i = 0; i < count; i++) {
    out_sizes[i] = items[i].status == Status::SUCCESS ? items[i].output_size : 0;
    if (statuses) statuses[i] = c_err(items[i].status);
  }
  return c_err(s);
}

nvcompZstdManagerHandle nvcomp_zstd_create_manager_v5(int level) {
  try {
    if (!is_valid_compression_level(level)) return nullptr;
    return (nvcompZstdManagerHandle) new ZstdBatchManager(CompressionConfig::from_level(level));
  } catch (...) {
    return nullptr;
  }
}
void nvcomp_zstd_destroy_manager_v5(nvcompZstdManagerHandle h) { delete static_cast<ZstdBatchManager *>(h); }
int nvcomp_zstd_compress_async_v5(nvcompZstdManagerHandle h, const void *in, size_t n, void *out, size_t *out_size, void *t, size_t ts, hipStream_t s) {
  auto *m = static_cast<ZstdBatchManager *>(h);
  if (!m) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(m->compress(in, n, out, out_size, t, ts, nullptr, 0, s));
}
int nvcomp_zstd_decompress_async_v5(nvcompZstdManagerHandle h, const void *in, size_t n, void *out, size_t *out_size, void *t, size_t ts, hipStream_t s) {
  auto *m = static_cast<ZstdBatchManager *>(h);
  if (!m) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(m->decompress(in, n, out, out_size, t, ts, s));
}
size_t nvcomp_zstd_get_compress_temp_size_v5(nvcompZstdManagerHandle h, size_t n) { return h ? static_cast<ZstdBatchManager *>(h)->get_compress_temp_size(n) : 0; }
size_t nvcomp_zstd_get_decompress_temp_size_v5(nvcompZstdManagerHandle h, size_t n) { return h ? static_cast<ZstdBatchManager *>(h)->get_decompress_temp_size(n) : 0; }
int nvcomp_zstd_get_metadata_v5(const void *d, size_t n, nvcomp_v5::NvcompV5Metadata *m, hipStream_t s) {
  return c_err(nvcomp_v5::get_metadata_async(d, n, m, s));
}

nvcomp_zstd_batch_manager_t *nvcomp_zstd_batch_create_v5(int level, unsigned int chunk_size, int enable_checksum) {
  try {
    if (!is_valid_compression_level(level)) return nullptr;
    nvcomp_v5::NvcompV5Options o;
    o.level = level;
    o.chunk_size = chunk_size ? chunk_size : 64 * 1024;
    o.enable_checksum = enable_checksum != 0;
    auto *m = new nvcomp_zstd_batch_manager_t;
    m->mgr.reset(new nvcomp_v5::NvcompV5BatchManager(o));
    return m;
  } catch (...) {
    return nullptr;
  }
}
void nvcomp_zstd_batch_destroy_v5(nvcomp_zstd_batch_manager_t *m) { delete m; }
size_t nvcomp_zstd_batch_get_compress_temp_size_v5(nvcomp_zstd_batch_manager_t *m, const size_t *sizes, size_t n) {
  return (m && m->mgr) ? m->mgr->get_compress_temp_size(sizes, n) : 0;
}
size_t nvcomp_zstd_batch_get_max_compressed_chunk_size_v5(nvcomp_zstd_batch_manager_t *m, size_t n) {
  return (m && m->mgr) ? m->mgr->get_max_compressed_chunk_size(n) : 0;
}
int nvcomp_zstd_batch_compress_async_v5(nvcomp_zstd_batch_manager_t *m, const void *const *in, const size_t *in_sizes, size_t n, void *const *out,
                                        size_t *out_sizes, void *t, size_t tb, hipStream_t s) {
  if (!m || !m->mgr) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(m->mgr->compress_async(in, in_sizes, n, out, out_sizes, t, tb, s));
}
size_t nvcomp_zstd_batched_compress_get_temp_size_v5(size_t n, size_t max_chunk) { return ZstdBatchManager::get_batch_device_temp_size(n, max_chunk); }
size_t nvcomp_zstd_batch_get_batched_temp_size_v5(nvcomp_zstd_batch_manager_t *m, size_t n, size_t max_chunk) {
  return (m && m->mgr) ? m->mgr->batch_manager().get_batch_device_temp_size_for(n, max_chunk) : 0;
}
int nvcomp_zstd_batch_set_dictionary_v5(nvcomp_zstd_batch_manager_t *m, cuda_zstd_dict_t *d) {
  if (!m || !m->mgr || !d || !d->dict) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(m->mgr->batch_manager().set_dictionary(*d->dict));
}
int nvcomp_zstd_batched_compress_async_v5(nvcomp_zstd_batch_manager_t *m, const void *const *d_in, const size_t *d_in_sizes, size_t max_chunk,
                                          size_t n, void *const *d_out, size_t *d_out_sizes, int *d_statuses, void *t, size_t tb, hipStream_t s) {
  if (!m || !m->mgr) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(m->mgr->batch_manager().compress_batch_device(d_in, d_in_sizes, max_chunk, n, d_out, d_out_sizes, d_statuses, t, tb, s));
}
size_t nvcomp_zstd_batched_compress_levels_get_temp_size_v5(size_t n, size_t max_chunk) {
  return ZstdBatchManager::get_batch_device_levels_temp_size(n, max_chunk);
}
int nvcomp_zstd_batched_compress_levels_async_v5(nvcomp_zstd_batch_manager_t *m, const void *const *d_in, const size_t *d_in_sizes,
                                                 const int *d_levels, size_t max_chunk, size_t n, void *const *d_out, size_t *d_out_sizes,
                                                 int *d_statuses, void *t, size_t tb, hipStream_t s) {
  if (!m || !m->mgr) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(
      m->mgr->batch_manager().compress_batch_device_levels(d_in, d_in_sizes, d_levels, max_chunk, n, d_out, d_out_sizes, d_statuses, t, tb, s));
}
size_t nvcomp_zstd_batch_get_batched_prefix_temp_size_v5(nvcomp_zstd_batch_manager_t *m, size_t n, size_t max_chunk) {
  return (m && m->mgr) ? m->mgr->batch_manager().get_batch_device_prefix_temp_size(n, max_chunk) : 0;
}
int nvcomp_zstd_batched_compress_prefix_async_v5(nvcomp_zstd_batch_manager_t *m, const void *const *d_in, const size_t *d_in_sizes,
                                                 const void *const *d_pre, const size_t *d_pre_sizes, size_t max_chunk, size_t n,
                                                 void *const *d_out, size_t *d_out_sizes, int *d_statuses, void *t, size_t tb, hipStream_t s) {
  if (!m || !m->mgr) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(m->mgr->batch_manager().compress_batch_device_prefix(d_in, d_in_sizes, d_pre, d_pre_sizes, max_chunk, n, d_out, d_out_sizes,
                                                                     d_statuses, t, tb, s));
}
int nvcomp_zstd_batched_decompress_prefix_async_v5(nvcomp_zstd_batch_manager_t *m, const void *const *d_in, const size_t *d_in_sizes,
                                                   const void *const *d_pre, const size_t *d_pre_sizes, const size_t *d_out_caps, size_t max_out,
                                                   size_t n, void *const *d_out, size_t *d_out_sizes, int *d_statuses, void *t, size_t tb,
                                                   hipStream_t s) {
  if (!m || !m->mgr) return c_err(Status::ERROR_INVALID_PARAMETER);
  if (n && (!d_pre || !d_pre_sizes)) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(m->mgr->batch_manager().decompress_batch_device_prefix(d_in, d_in_sizes, d_pre, d_pre_sizes, d_out_caps, max_out, n, d_out,
                                                                       d_out_sizes, d_statuses, t, tb, s));
}
// ---- dictionary sets (DESIGN.md §2 "A batch against a set of dictionaries") ----
int cuda_zstd_dict_set_create(const cuda_zstd_dict_t *const *dicts, size_t n, hipStream_t stream, cuda_zstd_dict_set_t **out) {
  if (out) *out = nullptr;
  if (!dicts || !out || n < 1 || n > ZH_DICTSET_MAX) return c_err(Status::ERROR_INVALID_PARAMETER);
  try {
    std::vector<const dictionary::Dictionary *> v(n);
    for (size_t i = 0; i < n; i++) {
      if (!dicts[i] || !dicts[i]->dict) return c_err(Status::ERROR_INVALID_PARAMETER);
      v[i] = dicts[i]->dict.get();
    }
    std::unique_ptr<DictionarySet> set;
    Status const s = DictionarySet::create(v.data(), n, stream, set);
    if (s != Status::SUCCESS) return c_err(s);
    auto *h = new cuda_zstd_dict_set_t;
    h->set = std::move(set);
    *out = h;
    return 0;
  } catch (...) {
    return c_err(Status::ERROR_OUT_OF_MEMORY);
  }
}
void cuda_zstd_dict_set_destroy(cuda_zstd_dict_set_t *set) { delete set; }
size_t cuda_zstd_dict_set_count(const cuda_zstd_dict_set_t *set) { return (set && set->set) ? set->set->count() : 0; }
int cuda_zstd_dict_set_find(const cuda_zstd_dict_set_t *set, unsigned int dict_id) { return (set && set->set) ? set->set->find(dict_id) : -1; }
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
int nvcomp_zstd_batch_set_dictionary_set_v5(nvcomp_zstd_batch_manager_t *m, cuda_zstd_dict_set_t *set) {
  if (!m || !m->mgr || (set && !set->set)) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(m->mgr->batch_manager().set_dictionary_set(set ? set->set.get() : nullptr));
}
size_t nvcomp_zstd_batch_get_batched_dicts_temp_size_v5(nvcomp_zstd_batch_manager_t *m, size_t n, size_t max_chunk) {
  return (m && m->mgr) ? m->mgr->batch_manager().get_batch_device_dicts_temp_size(n, max_chunk) : 0;
}
int nvcomp_zstd_batched_compress_dicts_async_v5(nvcomp_zstd_batch_manager_t *m, const void *const *d_in, const size_t *d_in_sizes,
                                                const int32_t *d_dict_index, size_t max_chunk, size_t n, void *const *d_out,
                                                size_t *d_out_sizes, int *d_statuses, void *t, size_t tb, hipStream_t s) {
  if (!m || !m->mgr) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(m->mgr->compress_dicts_async(d_in, d_in_sizes, d_dict_index, max_chunk, n, d_out, d_out_sizes, d_statuses, t, tb, s));
}
int nvcomp_zstd_batched_decompress_dicts_async_v5(nvcomp_zstd_batch_manager_t *m, const void *const *d_in, const size_t *d_in_sizes,
                                                  const int32_t *d_dict_index, const size_t *d_out_caps, size_t max_out, size_t n,
                                                  void *const *d_out, size_t *d_out_sizes, int *d_statuses, void *t, size_t tb, hipStream_t s) {
  if (!m || !m->mgr) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(m->mgr->decompress_dicts_async(d_in, d_in_sizes, d_dict_index, d_out_caps, max_out, n, d_out, d_out_sizes, d_statuses, t, tb, s));
}
size_t nvcomp_zstd_batch_get_decompress_temp_size_v5(nvcomp_zstd_batch_manager_t *m, const size_t *sizes, size_t n) {
  return (m && m->mgr) ? m->mgr->get_decompress_temp_size(sizes, n) : 0;
}
int nvcomp_zstd_batch_decompress_async_v5(nvcomp_zstd_batch_manager_t *m, const void *const *in, const size_t *in_sizes, size_t n, void *const *out,
                                          size_t *out_sizes, void *t, size_t tb, hipStream_t s) {
  if (!m || !m->mgr) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(m->mgr->decompress_async(in, in_sizes, n, out, out_sizes, t, tb, s));
}
size_t nvcomp_zstd_batched_decompress_get_temp_size_v5(size_t n, size_t max_out) {
  return ZstdBatchManager::get_batch_device_decompress_temp_size(n, max_out);
}
int nvcomp_zstd_batched_decompress_async_v5(nvcomp_zstd_batch_manager_t *m, const void *const *d_in, const size_t *d_in_sizes,
                                            const size_t *d_out_caps, size_t max_out, size_t n, void *const *d_out, size_t *d_out_sizes,
                                            int *d_statuses, void *t, size_t tb, hipStream_t s) {
  if (!m || !m->mgr) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(
      m->mgr->batch_manager().decompress_batch_device(d_in, d_in_sizes, d_out_caps, max_out, n, d_out, d_out_sizes, d_statuses, t, tb, s));
}
int nvcomp_zstd_batched_get_decompress_size_async_v5(nvcomp_zstd_batch_manager_t *m, const void *const *d_in, const size_t *d_in_sizes,
                                                     size_t *d_out_sizes, int *d_statuses, size_t n, hipStream_t s) {
  if (!m || !m->mgr) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(m->mgr->get_decompress_sizes_async(d_in, d_in_sizes, d_out_sizes, d_statuses, n, s));
}
int cuda_zstd_get_decompressed_sizes_async(cuda_zstd_manager_t *m, const void *const *d_ptrs, const size_t *d_sizes, size_t count,
                                           size_t *d_out_sizes, int *d_statuses, hipStream_t stream) {
  if (!m || !m->manager) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(m->manager->get_decompressed_sizes_async(d_ptrs, d_sizes, count, d_out_sizes, d_statuses, stream));
}

cuda_zstd_hybrid_engine_t *cuda_zstd_hybrid_create(const cuda_zstd_hybrid_config_t *c) {
  try {
    HybridConfig hc;
    if (c) {
      hc.mode = (HybridMode)c->mode;
      hc.cpu_size_threshold = c->cpu_size_threshold;
      hc.gpu_device_threshold = c->gpu_device_threshold;
      hc.compression_level = c->compression_level;
      hc.enable_profiling = c->enable_profiling != 0;
      hc.cpu_thread_count = c->cpu_thread_count;
      if (!is_valid_compression_level(hc.compression_level) || c->mode > 5) return nullptr;
    }
    auto *e = new cuda_zstd_hybrid_engine_t;
    e->engine.reset(new HybridEngine(hc));
    return e;
  } catch (...) {
    return nullptr;
  }
}
cuda_zstd_hybrid_engine_t *cuda_zstd_hybrid_create_default(void) { return cuda_zstd_hybrid_create(nullptr); }
void cuda_zstd_hybrid_destroy(cuda_zstd_hybrid_engine_t *e) { delete e; }
static void fill_result(cuda_zstd_hybrid_result_t *r, const HybridResult &h) {
  if (!r) return;
  r->backend_used = (unsigned)h.backend_used;
  r->input_location = (unsigned)h.input_location;
  r->output_location = (unsigned)h.output_location;
  r->total_time_ms = h.total_time_ms;
  r->transfer_time_ms = h.transfer_time_ms;
  r->compute_time_ms = h.compute_time_ms;
  r->throughput_mbps = h.throughput_mbps;
  r->input_bytes = h.input_bytes;
  r->output_bytes = h.output_bytes;
  r->compression_ratio = h.compression_ratio;
}
int cuda_zstd_hybrid_compress(cuda_zstd_hybrid_engine_t *e, const void *in, size_t n, void *out, size_t *out_size, unsigned il, unsigned ol,
                              cuda_zstd_hybrid_result_t *r, hipStream_t s) {
  if (!e || !e->engine || il > 3 || ol > 3) return c_err(Status::ERROR_INVALID_PARAMETER);
  HybridResult h;
  Status st = e->engine->compress(in, n, out, out_size, (DataLocation)il, (DataLocation)ol, &h, s);
  fill_result(r, h);
  return c_err(st);
}
int cuda_zstd_hybrid_decompress(cuda_zstd_hybrid_engine_t *e, const void *in, size_t n, void *out, size_t *out_size, unsigned il, unsigned ol,
                                cuda_zstd_hybrid_result_t *r, hipStream_t s) {
  if (!e || !e->engine || il > 3 || ol > 3) return c_err(Status::ERROR_INVALID_PARAMETER);
  HybridResult h;
  Status st = e->engine->decompress(in, n, out, out_size, (DataLocation)il, (DataLocation)ol, &h, s);
  fill_result(r, h);
  return c_err(st);
}
size_t cuda_zstd_hybrid_max_compressed_size(cuda_zstd_hybrid_engine_t *e, size_t n) { return (e && e->engine) ? e->engine->get_max_compressed_size(n) : 0; }
unsigned int cuda_zstd_hybrid_query_routing(cuda_zstd_hybrid_engine_t *e, size_t n, unsigned il, unsigned ol, int is_c) {
  if (!e || !e->engine) return 0;
  return (unsigned)e->engine->query_routing(n, (DataLocation)il, (DataLocation)ol, is_c != 0);
}

// Long-distance matching on a manager.  enable != 0: window_log / hash_log 0 select
// 27 / 20, what `zstd --long` takes.  enable == 0: matching off; a window_log / hash_log of 0 leaves
// the manager's value alone, another value is stored (the frame a caller compares against).
// Returns 2 for a window_log outside 16..31; the table size is clamped to 2^10..2^30 where it is used.
int cuda_zstd_set_long_distance(cuda_zstd_manager_t *m, int enable, unsigned window_log, unsigned hash_log) {
  if (!m || !m->manager) return c_err(Status::ERROR_INVALID_PARAMETER);
  CompressionConfig c = m->manager->get_config();
  if (enable && window_log == 0) window_log = 27;
  if (enable && hash_log == 0) hash_log = 20;
  if (window_log && (window_log < ZH_HIST_WINDOW_LOG || window_log > MAX_WINDOW_LOG)) return c_err(Status::ERROR_INVALID_PARAMETER);
  c.enable_ldm = enable != 0;
  if (window_log) c.window_log = window_log;
  if (hash_log) c.ldm_hash_log = hash_log;
  return c_err(m->manager->configure(c));
}
// CompressionConfig::dict_entropy (Dictionaries): the first block of a frame made with a
// formatted dictionary starts from its repcodes and may reuse its entropy tables.  Off by default;
// no effect without a dictionary, with raw content or on streaming-history frames.
int cuda_zstd_set_dict_entropy(cuda_zstd_manager_t *m, int enable) {
  if (!m || !m->manager) return c_err(Status::ERROR_INVALID_PARAMETER);
  CompressionConfig c = m->manager->get_config();
  c.dict_entropy = enable != 0;
  return c_err(m->manager->configure(c));
}
int nvcomp_zstd_batch_set_dict_entropy_v5(nvcomp_zstd_batch_manager_t *m, int enable) {
  if (!m || !m->mgr) return c_err(Status::ERROR_INVALID_PARAMETER);
  CompressionConfig c = m->mgr->batch_manager().get_config();
  c.dict_entropy = enable != 0;
  return c_err(m->mgr->batch_manager().configure(c));
}
// Content checksum of the manager's frames (0: none, the default)
int cuda_zstd_set_checksum(cuda_zstd_manager_t *m, int enable) {
  if (!m || !m->manager) return c_err(Status::ERROR_INVALID_PARAMETER);
  CompressionConfig c = m->manager->get_config();
  c.checksum = enable ? ChecksumPolicy::COMPUTE_NO_VERIFY : ChecksumPolicy::NO_COMPUTE_NO_VERIFY;
  return c_err(m->manager->configure(c));
}
// The finder's per-cell records {seg_start, seg_len, distance} (u32 each) for compress() of this
// device buffer; returns the number of records (cells), 0 when long-distance matching does not
// apply to the buffer, or -1 on error (capacity in records too small, workspace too small, ...)
long long cuda_zstd_hip_ldm_plan(cuda_zstd_manager_t *m, const void *d_src, size_t size, unsigned int *host_records, size_t capacity,
                                 void *workspace, size_t workspace_size, hipStream_t stream) {
  if (!m || !m->manager) return -1;
  size_t n = 0;
  Status const s = m->manager->ldm_plan(d_src, size, host_records, capacity, &n, workspace, workspace_size, stream);
  if (s != Status::SUCCESS) { (void)c_err(s); return -1; }
  return (long long)n;
}
// HIP events around the finder's two kernels: on = 1 starts recording; on = 0 stops and stores the
// summed milliseconds of the launches since then
void cuda_zstd_hip_ldm_profile(int on, double *ms) {
  double const t = zh::ldm_profile(on != 0);
  if (ms) *ms = t;
}
// HIP events around zh_window_update_kernel: on = 1 starts recording; on = 0 stops and stores the
// summed milliseconds of the launches since then
void cuda_zstd_hip_window_profile(int on, double *ms) {
  double const t = zh::window_profile(on != 0);
  if (ms) *ms = t;
}
void cuda_zstd_hip_profile_enable(int on) { zh::profile_enable(on != 0); }
int cuda_zstd_hip_profile_collect(double *ms3) { return zh::profile_collect(ms3); }

struct cuda_zstd_stream_t {
  std::unique_ptr<ZstdStreamingManager> m;
};
cuda_zstd_stream_t *cuda_zstd_stream_create(int level) {
  if (!is_valid_compression_level(level)) return nullptr;
  try {
    auto *h = new cuda_zstd_stream_t;
    h->m.reset(new ZstdStreamingManager(CompressionConfig::from_level(level)));
    return h;
  } catch (...) {
    return nullptr;
  }
}
void cuda_zstd_stream_destroy(cuda_zstd_stream_t *s) { delete s; }
int cuda_zstd_stream_compress_chunk(cuda_zstd_stream_t *s, const void *src, size_t n, void *dst, size_t *dst_size, int with_history, int last,
                                    hipStream_t stream) {
  if (!s || !s->m) return c_err(Status::ERROR_INVALID_PARAMETER);
  if (!with_history && !s->m->is_compression_initialized()) {
    Status st = s->m->init_compression(stream, n);
    if (st != Status::SUCCESS) return c_err(st);
  }
  return c_err(with_history ? s->m->compress_chunk_with_history(src, n, dst, dst_size, last != 0, stream)
                                             : s->m->compress_chunk(src, n, dst, dst_size, last != 0, stream));
}
int cuda_zstd_stream_decompress_chunk(cuda_zstd_stream_t *s, const void *src, size_t n, void *dst, size_t *dst_size, int *is_last,
                                      hipStream_t stream) {
  if (!s || !s->m) return c_err(Status::ERROR_INVALID_PARAMETER);
  bool l = false;
  Status st = s->m->decompress_chunk(src, n, dst, dst_size, &l, stream);
  if (is_last) *is_last = l ? 1 : 0;
  return c_err(st);
}
int cuda_zstd_stream_reset(cuda_zstd_stream_t *s) { return s && s->m ? c_err(s->m->reset()) : 2; }

// ---- many streams in one call (zh_stream.hip) -------------------------------------------------
// One device allocation made at create: the compress and the decode workspace, the window pairs of
// both directions (as ZstdStreamingManager keeps chist and dhist), per direction the current-half
// words and the prefix pointer / size arrays the prefix entries are called with, and a status array
// for callers that pass none.  A call is the prefix entry plus one window launch.
struct cuda_zstd_stream_batch_t {
  struct Dir {
    u8 *windows = nullptr;
    u32 *which = nullptr;
    const void **pre_ptrs = nullptr;
    size_t *pre_sizes = nullptr;
  };
  ZstdBatchManager mgr;
  size_t n = 0, max_chunk = 0, cws_bytes = 0, dws_bytes = 0;
  u8 *mem = nullptr, *cws = nullptr, *dws = nullptr;
  int *statuses = nullptr;
  Dir c, d;
  explicit cuda_zstd_stream_batch_t(int level) : mgr(CompressionConfig::from_level(level)) {}
  ~cuda_zstd_stream_batch_t() { if (mem) (void)hipFree(mem); }
  bool allocate() {
    cws_bytes = mgr.get_batch_device_prefix_temp_size(n, max_chunk);
    dws_bytes = ZstdBatchManager::get_batch_device_decompress_temp_size(n, max_chunk);
    size_t o = 0;
    auto take = [&o](size_t bytes) { size_t const at = o; o = align256(o + bytes); return at; };
    size_t const o_cws = take(cws_bytes), o_dws = take(dws_bytes), o_st = take(n * 4);
    size_t o_win[2], o_which[2], o_pp[2], o_ps[2];
    for (int k = 0; k < 2; k++) {
      o_win[k] = take(n * 2 * (size_t)ZH_STREAM_WINDOW);
      o_which[k] = take(n * 4);
      o_pp[k] = take(n * 8);
      o_ps[k] = take(n * 8);
    }
    if (hipMalloc(&mem, o) != hipSuccess) { mem = nullptr; return false; }
    cws = mem + o_cws;
    dws = mem + o_dws;
    statuses = (int *)(mem + o_st);
    Dir *dirs[2] = {&c, &d};
    for (int k = 0; k < 2; k++) {
      dirs[k]->windows = mem + o_win[k];
      dirs[k]->which = (u32 *)(mem + o_which[k]);
      dirs[k]->pre_ptrs = (const void **)(mem + o_pp[k]);
      dirs[k]->pre_sizes = (size_t *)(mem + o_ps[k]);
    }
    return true;
  }
  Status reset(hipStream_t stream) {
    for (Dir *x : {&c, &d})
      if (zh::window_reset_launch(x->windows, x->which, x->pre_ptrs, x->pre_sizes, (u32)n, stream) != hipSuccess) return Status::ERROR_CUDA_ERROR;
    return Status::SUCCESS;
  }
  Status advance(Dir &x, const void *const *chunk_ptrs, const size_t *chunk_sizes, const int *st, hipStream_t stream) {
    return zh::window_update_launch(x.windows, x.which, x.pre_ptrs, x.pre_sizes, chunk_ptrs, chunk_sizes, (const u32 *)st, (u32)n, stream) == hipSuccess
               ? Status::SUCCESS
               : Status::ERROR_CUDA_ERROR;
  }
};
cuda_zstd_stream_batch_t *cuda_zstd_stream_batch_create(int level, size_t num_streams, size_t max_chunk_bytes) {
  if (!is_valid_compression_level(level) || !num_streams || !max_chunk_bytes || num_streams > 0xFFFFFFFFull) return nullptr;
  try {
    std::unique_ptr<cuda_zstd_stream_batch_t> sb(new cuda_zstd_stream_batch_t(level));
    sb->n = num_streams;
    sb->max_chunk = max_chunk_bytes;
    if (ensure_kernels() != Status::SUCCESS || !sb->allocate()) return nullptr;
    if (sb->reset(nullptr) != Status::SUCCESS || hipStreamSynchronize(nullptr) != hipSuccess) return nullptr;
    return sb.release();
  } catch (...) {
    return nullptr;
  }
}
void cuda_zstd_stream_batch_destroy(cuda_zstd_stream_batch_t *sb) { delete sb; }
size_t cuda_zstd_stream_batch_max_compressed_chunk_size(cuda_zstd_stream_batch_t *sb) {
  return sb ? sb->mgr.get_max_compressed_size(sb->max_chunk) : 0;
}
int cuda_zstd_stream_batch_compress_async(cuda_zstd_stream_batch_t *sb, const void *const *d_in_ptrs, const size_t *d_in_sizes,
                                          void *const *d_out_ptrs, size_t *d_out_sizes, int *d_statuses, hipStream_t stream) {
  if (!sb || !d_in_ptrs || !d_in_sizes || !d_out_ptrs || !d_out_sizes) return c_err(Status::ERROR_INVALID_PARAMETER);
  int *const st = d_statuses ? d_statuses : sb->statuses;
  Status s = sb->mgr.compress_batch_device_prefix(d_in_ptrs, d_in_sizes, sb->c.pre_ptrs, sb->c.pre_sizes, sb->max_chunk, sb->n, d_out_ptrs,
                                                  d_out_sizes, st, sb->cws, sb->cws_bytes, stream);
  if (s == Status::SUCCESS) s = sb->advance(sb->c, d_in_ptrs, d_in_sizes, st, stream);
  return c_err(s);
}
int cuda_zstd_stream_batch_decompress_async(cuda_zstd_stream_batch_t *sb, const void *const *d_in_ptrs, const size_t *d_in_sizes,
                                            const size_t *d_out_caps, void *const *d_out_ptrs, size_t *d_out_sizes, int *d_statuses,
                                            hipStream_t stream) {
  if (!sb || !d_in_ptrs || !d_in_sizes || !d_out_ptrs || !d_out_sizes) return c_err(Status::ERROR_INVALID_PARAMETER);
  int *const st = d_statuses ? d_statuses : sb->statuses;
  Status s = sb->mgr.decompress_batch_device_prefix(d_in_ptrs, d_in_sizes, sb->d.pre_ptrs, sb->d.pre_sizes, d_out_caps, sb->max_chunk, sb->n,
                                                    d_out_ptrs, d_out_sizes, st, sb->dws, sb->dws_bytes, stream);
  if (s == Status::SUCCESS) s = sb->advance(sb->d, d_out_ptrs, d_out_sizes, st, stream);
  return c_err(s);
}
int cuda_zstd_stream_batch_reset(cuda_zstd_stream_batch_t *sb, hipStream_t stream) {
  return sb ? c_err(sb->reset(stream)) : c_err(Status::ERROR_INVALID_PARAMETER);
}

int cuda_zstd_write_metadata_frame(void *dst, size_t capacity, int level, size_t *written, hipStream_t stream) {
  return c_err(write_metadata_frame(dst, capacity, level, written, stream));
}
int cuda_zstd_extract_metadata(const void *src, size_t size, unsigned int *level, unsigned long long *usize, unsigned int *dict_id, int *has_ck) {
  NvcompMetadata m;
  Status s = extract_metadata(src, size, m);
  if (s == Status::SUCCESS) {
    if (level) *level = m.compression_level;
    if (usize) *usize = m.uncompressed_size;
    if (dict_id) *dict_id = m.dictionary_id;
    if (has_ck) *has_ck = m.checksum_policy != ChecksumPolicy::NO_COMPUTE_NO_VERIFY;
  }
  return c_err(s);
}

// ---- seekable streams (zh_seek.hip; format in zh_seek_format.h) -------------------------------
size_t cuda_zstd_seekable_max_size(size_t num_frames, size_t max_compressed_chunk_bytes, int with_checksums) {
  return num_frames * max_compressed_chunk_bytes + (size_t)zh_seek_table_bytes(num_frames, with_checksums);
}
size_t cuda_zstd_seekable_pack_get_temp_size(size_t num_frames) { return zh::seek_pack_temp_bytes(num_frames); }

int cuda_zstd_seekable_pack_async(const void *const *d_frame_ptrs, const size_t *d_frame_sizes, const int *d_frame_statuses,
                                  const void *const *d_uncompressed_ptrs, const size_t *d_uncompressed_sizes, size_t num_frames,
                                  size_t max_compressed_chunk_bytes, int with_checksums, void *d_out, size_t out_capacity, size_t *d_out_size,
                                  int *d_status, void *d_temp, size_t temp_bytes, hipStream_t stream) {
  if (!d_out || !d_out_size || !d_status || num_frames > ZH_SEEK_MAX_FRAMES) return c_err(Status::ERROR_INVALID_PARAMETER);
  if (num_frames && (!d_frame_ptrs || !d_frame_sizes || !d_uncompressed_sizes || max_compressed_chunk_bytes == 0 ||
                     (with_checksums && !d_uncompressed_ptrs)))
    return c_err(Status::ERROR_INVALID_PARAMETER);
  if (!d_temp || temp_bytes < zh::seek_pack_temp_bytes(num_frames)) return c_err(Status::ERROR_BUFFER_TOO_SMALL);
  hipError_t const e = zh::seek_pack_launch(d_frame_ptrs, d_frame_sizes, d_frame_statuses, d_uncompressed_ptrs, d_uncompressed_sizes, num_frames,
                                            max_compressed_chunk_bytes, with_checksums != 0, d_out, out_capacity, d_out_size, d_status, d_temp,
                                            stream);
  return e == hipSuccess ? 0 : c_err(Status::ERROR_CUDA_ERROR);
}

// The last 9 bytes of a stream in host or device memory, parsed on the host (the one small word
// the read and info calls fetch; the table itself stays where it is).
static int seek_fetch_footer(const void *buf, size_t size, bool dev, ZhSeekFooter &f, hipStream_t stream) {
  if (!buf) return 2;
  if (size < ZH_SEEK_OVERHEAD) return 6;
  u8 foot[ZH_SEEK_FOOTER];
  if (dev) {
    if (hipMemcpyAsync(foot, (const u8 *)buf + size - ZH_SEEK_FOOTER, ZH_SEEK_FOOTER, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
      return 4;
  } else {
    memcpy(foot, (const u8 *)buf + size - ZH_SEEK_FOOTER, ZH_SEEK_FOOTER);
  }
  return (int)zh_seek_parse_footer(foot, size, &f);
}

int cuda_zstd_seekable_info(const void *stream_buf, size_t size, size_t *num_frames, unsigned long long *total_uncompressed,
                            unsigned int *max_frame_uncompressed, int *has_checksums) {
  bool const dev = stream_buf && is_device_ptr(stream_buf);
  ZhSeekFooter f;
  int rc = seek_fetch_footer(stream_buf, size, dev, f, 0);
  if (rc) return rc;
  zh::SeekInfoRes r{};
  if (dev) {
    zh::SeekInfoRes *d_res = nullptr;
    if (hipMalloc((void **)&d_res, sizeof(r)) != hipSuccess) return 3;
    bool ok = hipMemsetAsync(d_res, 0, sizeof(r), 0) == hipSuccess && zh::seek_info_launch(stream_buf, size, (size_t)f.n, d_res, 0) == hipSuccess &&
              hipMemcpy(&r, d_res, sizeof(r), hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(d_res);
    if (!ok) return 4;
  } else {
    const u8 *const table = (const u8 *)stream_buf + (size - f.table);
    if (zh_seek_check_header(table, &f) != ZH_SEEK_OK) r.bad = 1;
    for (u64 i = 0; i < f.n; i++) {
      u64 const c = zh_seek_ld32(table + 8 + i * f.entry), d = zh_seek_ld32(table + 8 + i * f.entry + 4);
      if (!zh_seek_field_ok(c) || !zh_seek_field_ok(d)) { r.bad = 1; break; }
      r.total_c += c;
      r.total_u += d;
      r.max_d = std::max(r.max_d, (u32)d);
    }
  }
  if (r.bad || r.total_c + f.table != size) return 6;
  if (num_frames) *num_frames = (size_t)f.n;
  if (total_uncompressed) *total_uncompressed = r.total_u;
  if (max_frame_uncompressed) *max_frame_uncompressed = r.max_d;
  if (has_checksums) *has_checksums = (int)f.checksums;
  return 0;
}

// Temp of a read that decodes at most max_jobs frames (max_jobs = num_frames always suffices)
size_t cuda_zstd_seekable_read_get_temp_size_jobs(size_t num_frames, size_t max_jobs, size_t max_frame_uncompressed) {
  return zh::seek_read_fixed_bytes(num_frames) + zh::seek_read_bounce_bytes(max_frame_uncompressed) +
         ZstdBatchManager::get_batch_device_decompress_temp_size(std::min(max_jobs, num_frames), std::max<size_t>(max_frame_uncompressed, 1)) + 256;
}
size_t cuda_zstd_seekable_read_get_temp_size(size_t num_frames, size_t max_frame_uncompressed) {
  return cuda_zstd_seekable_read_get_temp_size_jobs(num_frames, num_frames, max_frame_uncompressed);
}

int cuda_zstd_seekable_read(nvcomp_zstd_batch_manager_t *mgr, const void *d_stream, size_t size, unsigned long long offset, size_t length,
                            void *d_out, size_t *written, int verify_checksums, void *d_temp, size_t temp_bytes, hipStream_t stream) {
  if (written) *written = 0;
  if (!mgr || !mgr->mgr || !d_stream || (length && !d_out)) return c_err(Status::ERROR_INVALID_PARAMETER);
  ZhSeekFooter f;
  int rc = seek_fetch_footer(d_stream, size, true, f, stream);
  if (rc) return rc;
  size_t const n = (size_t)f.n, fixed = zh::seek_read_fixed_bytes(n);
  if (!d_temp || temp_bytes < fixed + 256) return 7;  // nothing launched
  u8 *const base = aligned_base(d_temp);
  size_t const avail = temp_bytes - (size_t)(base - (u8 *)d_temp);
  if (zh::seek_index_launch(d_stream, size, n, f.entry, offset, length, d_out, base, stream) != hipSuccess) return 4;
  zh::SeekReadCtl ctl;
  if (hipMemcpyAsync(&ctl, base, sizeof(ctl), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return 4;
  if (ctl.status) return (int)ctl.status;
  if (ctl.njobs == 0) return 0;  // length 0 (a valid table, nothing to decode)
  // the decoder's workspace follows the bounce slots; sized now that the job count is known
  size_t const bounce = zh::seek_read_bounce_bytes(ctl.max_d), max_out = std::max<size_t>(ctl.max_d, 1);
  size_t const dec = ZstdBatchManager::get_batch_device_decompress_temp_size(ctl.njobs, max_out);
  if (ctl.njobs > n || avail < fixed + bounce + dec) return 7;  // the decoder is not launched
  zh::SeekJobs const j = zh::seek_read_jobs(base, n);
  Status const s = mgr->mgr->batch_manager().decompress_batch_device(j.in_ptrs, j.in_sizes, j.out_caps, max_out, ctl.njobs, j.out_ptrs, j.out_sizes,
                                                                     j.statuses, base + fixed + bounce, dec, stream);
  if (s != Status::SUCCESS) return c_err(s);
  if (zh::seek_trim_launch(d_stream, size, n, f.entry, ctl.njobs, offset, length, d_out, verify_checksums, base, stream) != hipSuccess) return 4;
  if (hipMemcpyAsync(&ctl, base, sizeof(ctl), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return 4;
  if (ctl.errkey != ~0ull) return (int)(ctl.errkey & 0xFFu);
  if (written) *written = length;
  return 0;
}

// Temp of a batched read whose ranges touch at most max_jobs frames with content
size_t cuda_zstd_seekable_read_ranges_get_temp_size(size_t num_frames, size_t num_ranges, size_t max_jobs, size_t max_frame_uncompressed) {
  size_t const jobs = std::min(max_jobs, num_frames);
  size_t const dec = ZstdBatchManager::get_batch_device_decompress_temp_size(jobs, std::max<size_t>(max_frame_uncompressed, 1));
  return zh::seek_ranges_layout(num_frames, num_ranges, jobs, max_frame_uncompressed, dec).total;
}

int cuda_zstd_seekable_read_ranges(nvcomp_zstd_batch_manager_t *mgr, const void *d_stream, size_t size, const unsigned long long *d_offsets,
                                   const size_t *d_lengths, void *const *d_out_ptrs, size_t num_ranges, size_t max_length, int verify_checksums,
                                   int *d_range_statuses, size_t *frames_decoded, void *d_temp, size_t temp_bytes, hipStream_t stream) {
  if (frames_decoded) *frames_decoded = 0;
  if (!mgr || !mgr->mgr || !d_stream) return c_err(Status::ERROR_INVALID_PARAMETER);
  if (num_ranges == 0) return 0;
  if (!d_offsets || !d_lengths || !d_out_ptrs || !d_range_statuses) return c_err(Status::ERROR_INVALID_PARAMETER);
  ZhSeekFooter f;
  int rc = seek_fetch_footer(d_stream, size, true, f, stream);
  if (rc) return rc;
  size_t const n = (size_t)f.n;
  // the part in front of the staging slots depends on the table and the ranges alone
  if (!d_temp || temp_bytes < zh::seek_ranges_layout(n, num_ranges, 0, 0, 0).staging + 256) return 7;  // nothing launched
  u8 *const base = aligned_base(d_temp);
  if (zh::seek_ranges_index_launch(d_stream, size, n, f.entry, d_offsets, d_lengths, num_ranges, max_length, base, stream) != hipSuccess) return 4;
  zh::SeekReadCtl ctl;
  if (hipMemcpyAsync(&ctl, base, sizeof(ctl), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return 4;
  if (ctl.status) return (int)ctl.status;
  // the staging slots and the decoder's workspace, sized now that the job count is known: the
  // buffer must be what get_temp_size asks for this many jobs
  size_t const max_out = std::max<size_t>(ctl.max_d, 1);
  size_t const dec = ctl.njobs ? ZstdBatchManager::get_batch_device_decompress_temp_size(ctl.njobs, max_out) : 0;
  ZhSeekRangesLayout const L = zh::seek_ranges_layout(n, num_ranges, ctl.njobs, ctl.max_d, dec);
  if (ctl.njobs > n || (ctl.njobs && temp_bytes < L.total)) return 7;  // the decoder is not launched
  if (ctl.njobs) {
    zh::SeekJobs const j = zh::seek_read_jobs(base, n);
    Status const s = mgr->mgr->batch_manager().decompress_batch_device(j.in_ptrs, j.in_sizes, j.out_caps, max_out, ctl.njobs, j.out_ptrs, j.out_sizes,
                                                                       j.statuses, base + L.dec, dec, stream);
    if (s != Status::SUCCESS) return c_err(s);
  }
  // (no range longer than the content is copied: the scatter grid is sized by the smaller bound)
  if (zh::seek_ranges_finish_launch(d_stream, size, n, f.entry, ctl.njobs, d_offsets, d_lengths, d_out_ptrs, num_ranges,
                                    (size_t)std::min<u64>(max_length, ctl.total_u), verify_checksums, d_range_statuses, base, stream) != hipSuccess)
    return 4;
  if (hipStreamSynchronize(stream) != hipSuccess) return 4;
  if (frames_decoded) *frames_decoded = ctl.njobs;
  return 0;
}

// ---- adaptive level selection (zh_adaptive.hip; the rule in zh_adaptive.h) ---------------------
size_t cuda_zstd_adaptive_get_temp_size(size_t num_chunks) { return num_chunks * ZH_AD_REC_WORDS * sizeof(u32); }

int cuda_zstd_adaptive_analyze_batch_async(const void *const *d_ptrs, const size_t *d_sizes, size_t num_chunks, size_t sample_bytes,
                                           int preference, cuda_zstd_adaptive_stats_t *d_stats, int *d_levels, void *d_temp,
                                           size_t temp_bytes, hipStream_t stream) {
  if (preference < 0 || preference > 2 || sample_bytes == 0) return c_err(Status::ERROR_INVALID_PARAMETER);
  if (num_chunks == 0) return 0;
  if (!d_ptrs || !d_sizes || !d_levels || !d_temp || ((uintptr_t)d_temp & 3u) || !zh::adaptive_grid(num_chunks, sample_bytes))
    return c_err(Status::ERROR_INVALID_PARAMETER);
  if (temp_bytes < cuda_zstd_adaptive_get_temp_size(num_chunks)) return c_err(Status::ERROR_BUFFER_TOO_SMALL);
  hipError_t const e = zh::adaptive_launch(d_ptrs, d_sizes, nullptr, 0, num_chunks, sample_bytes, preference, d_stats, d_levels, (u32 *)d_temp, stream);
  return e == hipSuccess ? 0 : c_err(Status::ERROR_CUDA_ERROR);
}

int cuda_zstd_adaptive_select_level(const void *d_data, size_t size, size_t sample_bytes, int preference, cuda_zstd_adaptive_stats_t *h_out,
                                    hipStream_t stream) {
  if (!h_out) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(adaptive_one(d_data, size, sample_bytes, preference, *h_out, stream));
}

int cuda_zstd_adaptive_finalize_host(const unsigned *hist256, unsigned sample_size, unsigned repeated_pairs, unsigned max_run_length,
                                     unsigned pattern_score, int preference, cuda_zstd_adaptive_stats_t *out) {
  if (!hist256 || !out || preference < 0 || preference > 2) return c_err(Status::ERROR_INVALID_PARAMETER);
  float const inv_n = sample_size ? 1.0f / (float)sample_size : 0.0f;
  float ent = 0.0f;
  u32 uniq = 0;
  for (u32 i = 0; i < 256; i++) {
    uniq += hist256[i] != 0;
    ent += zh_adaptive_entropy_term(hist256[i], inv_n);
  }
  zh_adaptive_decide(sample_size, repeated_pairs, max_run_length, pattern_score, uniq, ent, preference, out);
  return 0;
}

const char *cuda_zstd_hip_version(void) { return "cuda_zstd_hip 0.2.0 (gfx950)"; }
unsigned int cuda_zstd_hip_kernel_lds_bytes(int which) { return which == 0 ? zh::lz_lds_bytes() : zh::entropy_lds_bytes(); }

}  // extern "C"

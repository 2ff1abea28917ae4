// zh_host_base.cpp — host runtime, base: status strings, the error context, CompressionConfig and
// the level table, the host libzstd bridge, copy_any, the frame probe and the metadata helpers.
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
#include "zh_host.h"

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
Status noted(Status s, const char *fn, int line) {
  if (s != Status::SUCCESS) log_error(ErrorContext(s, __FILE__, line, fn));
  return s;
}

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
}  // namespace
size_t cpu_compress_bound(size_t n) { return libzstd().ok ? libzstd().compressBound(n) : 0; }

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

namespace {
std::once_flag g_init_flag;
hipError_t g_init_err = hipSuccess;
}  // namespace
Status ensure_kernels() {
  std::call_once(g_init_flag, [] { g_init_err = zh::init_kernels(); });
  return g_init_err == hipSuccess ? Status::SUCCESS : Status::ERROR_CUDA_ERROR;
}

// Frame header fields of the first zstd frame in a buffer, after any skippable frames (the
// reference parse_zstd_frame_header skips them the same way, src/cuda_zstd_manager.cu:875-900);
// *meta_level = the level of a metadata frame written by write_metadata_frame, else -1.
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

}  // namespace cuda_zstd

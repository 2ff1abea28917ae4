// zh_host.h — what the host runtime's translation units share (zh_host_*.cpp).  Internal: every
// function here is hidden from the library's dynamic symbols; the layouts, the dictionary objects
// and the managers' Impl classes stay private to the one file that owns them.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "cuda_zstd_adaptive.h"
#include "cuda_zstd_hybrid.h"
#include "cuda_zstd_manager.h"
#include "cuda_zstd_nvcomp.h"
#include "zh_launch.h"

#define ZH_INTERNAL __attribute__((visibility("hidden")))  // a helper member of an exported class: not a dynamic symbol
#pragma GCC visibility push(hidden)
namespace cuda_zstd {

// a public entry point's result: failures go to the last-error slot (and the callback)
Status noted(Status s, const char *fn, int line);
#define ZH_NOTED(s) noted((s), __func__, __LINE__)

// host libzstd, opened once (the reference's CPU route; FORCE_CPU + decompress)
size_t cpu_compress_bound(size_t n);  // ZSTD_compressBound, 0 without a libzstd
Status cpu_compress(const void *in, size_t n, void *out, size_t *out_size, int level, hipStream_t stream);
Status cpu_decompress(const void *in, size_t n, void *out, size_t *out_size, hipStream_t stream);

bool is_device_ptr(const void *p);
Status copy_any(void *dst, const void *src, size_t n, hipStream_t stream);
Status ensure_kernels();

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
// A caller's temp buffer starts at its first 256-byte boundary (every layout's total holds the slack)
inline u8 *aligned_base(void *temp) { return (u8 *)align256((uintptr_t)temp); }
// Regions of one buffer, each starting at a 256-byte boundary (0 bytes: an empty region)
struct Carve {
  size_t o = 0;
  size_t take(size_t bytes) {
    size_t const at = o;
    o = align256(o + bytes);
    return at;
  }
};

// Frame header fields of the first zstd frame in a buffer, after any skippable frames
struct FrameProbe {
  u64 content = 0;
  bool has_content = false, checksum = false;
  u32 dict_id = 0, window_log = 0;
  int meta_level = -1;
  size_t frame_offset = 0;
};
Status probe_frame(const void *data, size_t n, FrameProbe &f);

// one device buffer through the adaptive kernels (zh_host_adaptive.cpp)
Status adaptive_one(const void *d_data, size_t size, size_t sample_bytes, int preference, cuda_zstd_adaptive_stats_t &out, hipStream_t stream);

namespace dictionary {
// the device trainer (zh_host_train.cpp)
Status train_groups_device(const u8 *d_corpus, const size_t *sizes, size_t n, const size_t *counts, size_t ng, size_t dict_size, u32 k, u32 d,
                           void *temp, size_t temp_bytes, bool own_temp, hipStream_t stream, std::vector<std::vector<u8>> &contents);
Status train_device(const u8 *d_corpus, const size_t *sizes, size_t n, size_t dict_size, u32 k, u32 d, void *temp, size_t temp_bytes,
                    bool own_temp, hipStream_t stream, std::vector<u8> &content);
}  // namespace dictionary

// every C entry's Status -> the reference's int codes; failures also go to the last-error slot
inline int c_err(Status s) { return nvcomp_v5::status_to_nvcomp_error(s == Status::SUCCESS ? s : noted(s, "C API", 0)); }

}  // namespace cuda_zstd
#pragma GCC visibility pop

// ---- the C ABI's opaque handles ----
struct cuda_zstd_manager_t { std::unique_ptr<cuda_zstd::ZstdBatchManager> manager; };
// the handle owns the bytes; `dict` is the reference-shaped view of them (its copy operations
// would malloc, so it is never copied here)
struct cuda_zstd_dict_t {
  std::vector<u8> bytes;
  std::unique_ptr<cuda_zstd::dictionary::Dictionary> dict;
  void set(std::vector<u8> &&b, u32 id) {
    bytes = std::move(b);
    dict.reset(new cuda_zstd::dictionary::Dictionary);
    dict->raw_content = bytes.data();
    dict->raw_size = (u32)bytes.size();
    dict->header.dictionary_id = id;
    dict->header.raw_content_size = (u32)bytes.size();
  }
};
struct cuda_zstd_dict_set_t { std::unique_ptr<cuda_zstd::DictionarySet> set; };
struct nvcomp_zstd_batch_manager_t { std::unique_ptr<cuda_zstd::nvcomp_v5::NvcompV5BatchManager> mgr; };

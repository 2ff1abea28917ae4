// zh_host_nvcomp.cpp — host runtime, the NVCOMP v5 layer.
#include "zh_host.h"

namespace cuda_zstd {
// NVCOMP v5 layer (reference src/cuda_zstd_nvcomp.cpp)
namespace nvcomp_v5 {
// Status <-> the nvcomp-style int codes (reference src/cuda_zstd_nvcomp.cpp:75-96); any other Status is 1, any other code ERROR_GENERIC
static const struct { Status s; int e; } kCodes[] = {
    {Status::SUCCESS, 0},          {Status::ERROR_INVALID_PARAMETER, 2}, {Status::ERROR_OUT_OF_MEMORY, 3},    {Status::ERROR_CUDA_ERROR, 4},
    {Status::ERROR_CORRUPT_DATA, 6}, {Status::ERROR_BUFFER_TOO_SMALL, 7},  {Status::ERROR_CHECKSUM_FAILED, 10}, {Status::ERROR_COMPRESSION, 12}};
int status_to_nvcomp_error(Status s) {
  for (auto const &c : kCodes)
    if (c.s == s) return c.e;
  return 1;
}
Status nvcomp_error_to_status(int e) {
  for (auto const &c : kCodes)
    if (c.e == e) return c.s;
  return Status::ERROR_GENERIC;
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

}  // namespace cuda_zstd

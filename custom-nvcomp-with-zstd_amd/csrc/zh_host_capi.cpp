// zh_host_capi.cpp — host runtime, the C ABI of the managers, dictionaries and dictionary sets
// (reference src/cuda_zstd_c_api.cpp:10-209, src/cuda_zstd_nvcomp.cpp:766-840); the other subsystems' C
// entries live with them.
#include "zh_dict.h"
#include "zh_host.h"

using namespace cuda_zstd;

struct cuda_zstd_stream_t {
  std::unique_ptr<ZstdStreamingManager> m;
};

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
// cuda_zstd_compress_batch / cuda_zstd_decompress_batch: the arrays as BatchItems, the batch call,
// sizes and codes written back (a failed item's size: left alone by compress, 0 from the decoder)
static int c_batch(cuda_zstd_manager_t *m, bool comp, const void *const *in_ptrs, const size_t *in_sizes, size_t count, void *const *out_ptrs,
                   size_t *out_sizes, int *statuses, void *ws, size_t ws_size, hipStream_t stream) {
  if (!m || !m->manager || (count && (!in_ptrs || !in_sizes || !out_ptrs || !out_sizes))) return c_err(Status::ERROR_INVALID_PARAMETER);
  std::vector<BatchItem> items(count);
  for (size_t i = 0; i < count; i++) {
    items[i].input_ptr = (void *)in_ptrs[i];
    items[i].output_ptr = out_ptrs[i];
    items[i].input_size = in_sizes[i];
    items[i].output_size = out_sizes[i];
  }
  Status s = comp ? m->manager->compress_batch(items, ws, ws_size, stream) : m->manager->decompress_batch(items, ws, ws_size, stream);
  for (size_t i = 0; i < count; i++) {
    if (items[i].status == Status::SUCCESS) out_sizes[i] = items[i].output_size;
    else if (!comp) out_sizes[i] = 0;
    if (statuses) statuses[i] = c_err(items[i].status);
  }
  return c_err(s);
}
int cuda_zstd_compress_batch(cuda_zstd_manager_t *m, const void *const *in_ptrs, const size_t *in_sizes, size_t count, void *const *out_ptrs,
                             size_t *out_sizes, int *statuses, void *ws, size_t ws_size, hipStream_t stream) {
  return c_batch(m, true, in_ptrs, in_sizes, count, out_ptrs, out_sizes, statuses, ws, ws_size, stream);
}
size_t cuda_zstd_get_batch_decompress_workspace_size(cuda_zstd_manager_t *m, const size_t *sizes, size_t count) {
  if (!m || !m->manager || (!sizes && count)) return 0;
  return m->manager->get_batch_decompress_temp_size(std::vector<size_t>(sizes, sizes + count));
}
int cuda_zstd_decompress_batch(cuda_zstd_manager_t *m, const void *const *in_ptrs, const size_t *in_sizes, size_t count, void *const *out_ptrs,
                               size_t *out_sizes, int *statuses, void *ws, size_t ws_size, hipStream_t stream) {
  return c_batch(m, false, in_ptrs, in_sizes, count, out_ptrs, out_sizes, statuses, ws, ws_size, stream);
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

const char *cuda_zstd_hip_version(void) { return "cuda_zstd_hip 0.2.0 (gfx950)"; }
unsigned int cuda_zstd_hip_kernel_lds_bytes(int which) { return which == 0 ? zh::lz_lds_bytes() : zh::entropy_lds_bytes(); }

}  // extern "C"

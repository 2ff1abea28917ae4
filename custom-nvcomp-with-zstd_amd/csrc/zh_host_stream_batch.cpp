// zh_host_stream_batch.cpp — host runtime, the stream-batch driver (C entries).
#include "zh_host.h"
#include "zh_stream_window.h"

using namespace cuda_zstd;

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
    Carve cv;
    size_t const o_cws = cv.take(cws_bytes), o_dws = cv.take(dws_bytes), o_st = cv.take(n * 4);
    size_t o_win[2], o_which[2], o_pp[2], o_ps[2];
    for (int k = 0; k < 2; k++) {
      o_win[k] = cv.take(n * 2 * (size_t)ZH_STREAM_WINDOW);
      o_which[k] = cv.take(n * 4);
      o_pp[k] = cv.take(n * 8);
      o_ps[k] = cv.take(n * 8);
    }
    if (hipMalloc(&mem, cv.o) != hipSuccess) { mem = nullptr; return false; }
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
extern "C" {
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

}  // extern "C"

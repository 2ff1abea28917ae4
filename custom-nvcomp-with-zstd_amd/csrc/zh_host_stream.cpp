// zh_host_stream.cpp — host runtime, the streaming manager.
#include "zh_host.h"

namespace cuda_zstd {
// Streaming manager (reference src/cuda_zstd_manager.cu:6043-6455).  compress_chunk: each chunk
// an independent frame (:6306-6310).  compress_chunk_with_history: the chunk is compressed with
// the preceding stream bytes (a 64 KiB device window, the most K1 can stage) as raw-content
// history, as the reference passes its window to compress() as a dictionary (:6327-6418).
// decompress_chunk keeps the same window of decoded bytes and hands it to the decoder, so
// chunks of either kind decode in stream order.
namespace {
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
  // One chunk as a frame of its own, or (hist) against the stream window.  The window, once it
  // exists, follows every chunk, so a later chunk with history sees these bytes: its next state
  // goes to the other buffer while this chunk may read the current one, and the copy is enqueued
  // first, so the compress call's final synchronisation covers it.
  ZH_INTERNAL Status compress_chunk(bool hist, const void *in, size_t n, void *out, size_t *out_size, hipStream_t stream) {
    Status s = ensure_ws(mgr.get_compress_temp_size(n));
    if (s != Status::SUCCESS) return s;
    bool const win = chist.buf[0] != nullptr;  // (hist: always)
    if (win) {
      s = chist.stage(in, n, stream);
      if (s != Status::SUCCESS) return s;
    }
    s = hist ? mgr.compress_with_history(in, n, out, out_size, ws, ws_size, chist.data(), chist.n, stream)
             : mgr.compress(in, n, out, out_size, ws, ws_size, nullptr, 0, stream);
    if (s == Status::SUCCESS && win) chist.commit();
    else if (win) (void)hipStreamSynchronize(stream);  // (an early error return: the copy still reads `in`)
    return s;
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
  return pimpl_->compress_chunk(false, in, n, out, out_size, stream);
}
Status ZstdStreamingManager::compress_chunk_with_history(const void *in, size_t n, void *out, size_t *out_size, bool, hipStream_t stream) {
  if (!in || !out || !out_size) return Status::ERROR_INVALID_PARAMETER;
  if (!pimpl_->comp || !pimpl_->chist.buf[0]) {  // auto-initialise, as the reference does
    Status s = init_compression_with_history(stream, n);
    if (s != Status::SUCCESS) return s;
  }
  return pimpl_->compress_chunk(true, in, n, out, out_size, stream);
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

std::unique_ptr<ZstdStreamingManager> create_streaming_manager(int level) {
  return std::unique_ptr<ZstdStreamingManager>(new ZstdStreamingManager(CompressionConfig::from_level(level)));
}
}  // namespace cuda_zstd

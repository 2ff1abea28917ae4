// zh_host_hybrid.cpp — host runtime, HybridEngine with its C entries.
#include "zh_host.h"

namespace cuda_zstd {
// HybridEngine (reference src/cuda_zstd_hybrid.cu)
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

  // compress (comp) or decompress one buffer: the routing, the staging of host buffers through
  // device memory for the device pipeline, the timing, the stats and the HybridResult
  ZH_INTERNAL Status routed(const HybridEngine &eng, bool comp, const void *in, size_t n, void *out, size_t *out_size, DataLocation il,
                            DataLocation ol, HybridResult *res, hipStream_t stream) {
    if (il == DataLocation::UNKNOWN) il = detect_location(in);
    if (ol == DataLocation::UNKNOWN) ol = detect_location(out);
    auto t0 = std::chrono::steady_clock::now();
    ExecutionBackend be = eng.query_routing(n, il, ol, comp);
    Status s;
    if (be == ExecutionBackend::CPU_LIBZSTD) {
      s = comp ? cpu_compress(in, n, out, out_size, config.compression_level, stream) : cpu_decompress(in, n, out, out_size, stream);
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
        if (hipMalloc(&tmp_out, comp ? cap : std::max<size_t>(cap, 1)) != hipSuccess) s = Status::ERROR_OUT_OF_MEMORY;
        dout = tmp_out;
      }
      size_t need = comp ? mgr.get_compress_temp_size(n) : mgr.get_decompress_temp_size(n);
      if (s == Status::SUCCESS && hipMalloc(&ws, need) != hipSuccess) s = Status::ERROR_OUT_OF_MEMORY;
      if (s == Status::SUCCESS)
        s = comp ? mgr.compress(din, n, dout, out_size, ws, need, nullptr, 0, stream) : mgr.decompress(din, n, dout, out_size, ws, need, stream);
      if (s == Status::SUCCESS && tmp_out) s = copy_any(out, tmp_out, *out_size, stream);
      if (tmp_in) (void)hipFree(tmp_in);
      if (tmp_out) (void)hipFree(tmp_out);
      if (ws) (void)hipFree(ws);
    }
    double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (s == Status::SUCCESS) {
      if (comp) stats.input_bytes += n;
      (comp ? stats.output_bytes : stats.bytes_decompressed) += *out_size;
      (comp ? stats.compression_time_ms : stats.decompression_time_ms) += ms;
      profile(be, comp, comp ? n : *out_size, ms);
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
    if (res && comp) {  // (compress alone reports these)
      res->compression_ratio = (s == Status::SUCCESS && *out_size) ? (float)n / *out_size : 0.f;
      res->throughput_mbps = ms > 0 ? n / 1e6 / (ms / 1e3) : 0;
      res->routing_reason = be == ExecutionBackend::CPU_LIBZSTD ? "cpu (libzstd)" : "gpu (gfx950 kernels)";
    }
    return s;
  }

  // compress_batch / decompress_batch: every item through the engine's call, its result filled; true when all succeeded
  ZH_INTERNAL bool routed_batch(HybridEngine &eng, bool comp, const void *const *inputs, const size_t *sizes, void **outputs, size_t *out_sizes,
                                size_t count, DataLocation il, DataLocation ol, BatchRoutingResult *results, hipStream_t stream) {
    bool ok = true;
    for (size_t i = 0; i < count; i++) {
      HybridResult r;
      Status s = comp ? eng.compress(inputs[i], sizes[i], outputs[i], &out_sizes[i], il, ol, &r, stream)
                      : eng.decompress(inputs[i], sizes[i], outputs[i], &out_sizes[i], il, ol, &r, stream);
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
    return ok;
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
  HybridConfig c = pimpl_->config;
  c.compression_level = level;
  return configure(c);
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
  return std::max(estimate_compressed_size(n, pimpl_->config.compression_level), cpu_compress_bound(n));
}
CompressionStats HybridEngine::get_stats() const { return pimpl_->stats; }
void HybridEngine::reset_stats() { pimpl_->stats = CompressionStats{}; }

// Routing as the reference's (src/cuda_zstd_hybrid.cu:836-905): libzstd for host data / FORCE_CPU, the
// gfx950 kernels for device data (host buffers staged through HBM when forced)
Status HybridEngine::compress(const void *in, size_t n, void *out, size_t *out_size, DataLocation il, DataLocation ol, HybridResult *res,
                              hipStream_t stream) {
  if (!in || !out || !out_size || n == 0) return Status::ERROR_INVALID_PARAMETER;
  return ZH_NOTED(pimpl_->routed(*this, true, in, n, out, out_size, il, ol, res, stream));
}
Status HybridEngine::decompress(const void *in, size_t n, void *out, size_t *out_size, DataLocation il, DataLocation ol, HybridResult *res,
                                hipStream_t stream) {
  if (!in || !out || !out_size || n < 4) return Status::ERROR_INVALID_PARAMETER;
  return ZH_NOTED(pimpl_->routed(*this, false, in, n, out, out_size, il, ol, res, stream));
}

// reference src/cuda_zstd_hybrid.cu:912-992: items one by one through the routing; per-item
// BatchRoutingResult; ERROR_COMPRESSION / ERROR_DECOMPRESSION when any item failed
Status HybridEngine::compress_batch(const void *const *inputs, const size_t *sizes, void **outputs, size_t *out_sizes, size_t count,
                                    DataLocation il, DataLocation ol, BatchRoutingResult *results, hipStream_t stream) {
  if (!inputs || !sizes || !outputs || !out_sizes || count == 0) return ZH_NOTED(Status::ERROR_INVALID_PARAMETER);
  return pimpl_->routed_batch(*this, true, inputs, sizes, outputs, out_sizes, count, il, ol, results, stream) ? Status::SUCCESS
                                                                                                             : ZH_NOTED(Status::ERROR_COMPRESSION);
}
Status HybridEngine::decompress_batch(const void *const *inputs, const size_t *sizes, void **outputs, size_t *out_sizes, size_t count,
                                      DataLocation il, DataLocation ol, BatchRoutingResult *results, hipStream_t stream) {
  if (!inputs || !sizes || !outputs || !out_sizes || count == 0) return ZH_NOTED(Status::ERROR_INVALID_PARAMETER);
  return pimpl_->routed_batch(*this, false, inputs, sizes, outputs, out_sizes, count, il, ol, results, stream) ? Status::SUCCESS
                                                                                                              : ZH_NOTED(Status::ERROR_DECOMPRESSION);
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

}  // namespace cuda_zstd

using namespace cuda_zstd;

struct cuda_zstd_hybrid_engine_t { std::unique_ptr<HybridEngine> engine; };

extern "C" {
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
static int c_routed(cuda_zstd_hybrid_engine_t *e, bool comp, const void *in, size_t n, void *out, size_t *out_size, unsigned il, unsigned ol,
                    cuda_zstd_hybrid_result_t *r, hipStream_t s) {
  if (!e || !e->engine || il > 3 || ol > 3) return c_err(Status::ERROR_INVALID_PARAMETER);
  HybridResult h;
  Status st = comp ? e->engine->compress(in, n, out, out_size, (DataLocation)il, (DataLocation)ol, &h, s)
                   : e->engine->decompress(in, n, out, out_size, (DataLocation)il, (DataLocation)ol, &h, s);
  fill_result(r, h);
  return c_err(st);
}
int cuda_zstd_hybrid_compress(cuda_zstd_hybrid_engine_t *e, const void *in, size_t n, void *out, size_t *out_size, unsigned il, unsigned ol,
                              cuda_zstd_hybrid_result_t *r, hipStream_t s) {
  return c_routed(e, true, in, n, out, out_size, il, ol, r, s);
}
int cuda_zstd_hybrid_decompress(cuda_zstd_hybrid_engine_t *e, const void *in, size_t n, void *out, size_t *out_size, unsigned il, unsigned ol,
                                cuda_zstd_hybrid_result_t *r, hipStream_t s) {
  return c_routed(e, false, in, n, out, out_size, il, ol, r, s);
}
size_t cuda_zstd_hybrid_max_compressed_size(cuda_zstd_hybrid_engine_t *e, size_t n) { return (e && e->engine) ? e->engine->get_max_compressed_size(n) : 0; }
unsigned int cuda_zstd_hybrid_query_routing(cuda_zstd_hybrid_engine_t *e, size_t n, unsigned il, unsigned ol, int is_c) {
  if (!e || !e->engine) return 0;
  return (unsigned)e->engine->query_routing(n, (DataLocation)il, (DataLocation)ol, is_c != 0);
}

}  // extern "C"

// ldm_paths.cpp — which entry points of ZstdBatchManager take CompressionConfig::enable_ldm and
// which ignore it (tests/test_gpu_ldm.py runs it).  usage: ldm_paths <file>
// <file> = one buffer of more than 64 KiB with a repeat further back than 64 KiB.  Two managers,
// level 3, window 2^20, one with enable_ldm and one without:
//   compress()                         the flag shrinks the frame; stats count one block per cell
//   compress_batch() of that one item  succeeds with get_batch_compress_temp_size() and gives the
//                                      frame the manager without the flag gives
//   compress_batch(), cpu_threshold    a small item takes the host route, the big one is the only
//                                      device item left: same frames with and without the flag
//   compress_with_history()            with a history: same frame with and without the flag
//   compress() with a dictionary       per-call raw-content dictionary: same frame
// Prints "ldm paths OK" and returns 0 when all of that holds.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "cuda_zstd_manager.h"

using namespace cuda_zstd;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); return 2; } } while (0)
#define REQ(c, ...) do { if (!(c)) { fprintf(stderr, "line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return 3; } } while (0)

static CompressionConfig config(bool ldm, u32 cpu_threshold) {
  CompressionConfig c = CompressionConfig::from_level(3);
  c.window_log = 20;
  c.enable_ldm = ldm;
  c.cpu_threshold = cpu_threshold;
  return c;
}

static std::vector<char> fetch(const void *d, size_t n) {
  std::vector<char> h(n);
  (void)hipMemcpy(h.data(), d, n, hipMemcpyDeviceToHost);
  return h;
}

int main(int argc, char **argv) {
  if (argc < 2) return 1;
  std::ifstream f(argv[1], std::ios::binary);
  std::vector<char> in((std::istreambuf_iterator<char>(f)), {});
  size_t const n = in.size(), small_n = 1000;
  REQ(n > 65536 + small_n, "input too small");
  size_t const cap = estimate_compressed_size(n, 3);
  void *d_in, *d_small, *d_out[2], *d_out_small[2], *d_hist, *d_temp;
  CK(hipMalloc(&d_in, n));
  CK(hipMemcpy(d_in, in.data(), n, hipMemcpyHostToDevice));
  CK(hipMalloc(&d_small, small_n));
  CK(hipMemcpy(d_small, in.data(), small_n, hipMemcpyHostToDevice));
  CK(hipMalloc(&d_hist, 40000));
  CK(hipMemcpy(d_hist, in.data() + 1234, 40000, hipMemcpyHostToDevice));
  for (int k = 0; k < 2; k++) { CK(hipMalloc(&d_out[k], cap)); CK(hipMalloc(&d_out_small[k], cap)); }

  // ---- compress(): the flag is taken
  std::vector<char> plain[2];
  for (int k = 0; k < 2; k++) {
    ZstdBatchManager m(config(k == 1, 0));
    size_t const ts = m.get_compress_temp_size(n);
    CK(hipMalloc(&d_temp, ts));
    size_t sz = cap;
    Status st = m.compress(d_in, n, d_out[k], &sz, d_temp, ts, nullptr, 0, 0);
    REQ(st == Status::SUCCESS, "compress (ldm %d): %s", k, status_to_string(st));
    plain[k] = fetch(d_out[k], sz);
    REQ(m.get_stats().num_blocks == (n + 32767) / 32768, "ldm %d: %llu blocks counted", k, (unsigned long long)m.get_stats().num_blocks);
    CK(hipFree(d_temp));
  }
  REQ(plain[1].size() + 30000 < plain[0].size(), "the flag did not shrink compress()'s frame: %zu vs %zu", plain[1].size(), plain[0].size());

  // ---- compress_batch() of the one item, and of a small + the big item with a cpu_threshold
  for (u32 thr : {0u, 49152u}) {
    std::vector<char> got[2][2];
    for (int k = 0; k < 2; k++) {
      ZstdBatchManager m(config(k == 1, thr));
      std::vector<BatchItem> items;
      std::vector<size_t> sizes;
      if (thr) {
        BatchItem s;
        s.input_ptr = d_small; s.input_size = small_n; s.output_ptr = d_out_small[k]; s.output_size = cap;
        items.push_back(s);
        sizes.push_back(small_n);
      }
      BatchItem b;
      b.input_ptr = d_in; b.input_size = n; b.output_ptr = d_out[k]; b.output_size = cap;
      items.push_back(b);
      sizes.push_back(n);
      size_t const ts = m.get_batch_compress_temp_size(sizes);
      if (k == 1) REQ(ts == ZstdBatchManager(config(false, thr)).get_batch_compress_temp_size(sizes), "the batch workspace size depends on the flag");
      CK(hipMalloc(&d_temp, ts));
      Status st = m.compress_batch(items, d_temp, ts, 0);
      REQ(st == Status::SUCCESS, "compress_batch (ldm %d, threshold %u): %s", k, thr, status_to_string(st));
      for (size_t i = 0; i < items.size(); i++) {
        REQ(items[i].status == Status::SUCCESS, "item %zu (ldm %d, threshold %u): %s", i, k, thr, status_to_string(items[i].status));
        got[k][i] = fetch(items[i].output_ptr, items[i].output_size);
      }
      CK(hipFree(d_temp));
    }
    for (int i = 0; i < (thr ? 2 : 1); i++) REQ(got[0][i] == got[1][i], "threshold %u item %d: the batch frame depends on the flag", thr, i);
    REQ(got[0][thr ? 1 : 0] == plain[0], "threshold %u: the batch frame of the big item is not compress()'s without the flag", thr);
  }

  // ---- history and per-call dictionary: the flag is ignored
  std::vector<char> hist[2], dict[2];
  for (int k = 0; k < 2; k++) {
    ZstdBatchManager m(config(k == 1, 0));
    size_t const ts = m.get_compress_temp_size(n);
    CK(hipMalloc(&d_temp, ts));
    size_t sz = cap;
    Status st = m.compress_with_history(d_in, n, d_out[k], &sz, d_temp, ts, d_hist, 40000, 0);
    REQ(st == Status::SUCCESS, "compress_with_history (ldm %d): %s", k, status_to_string(st));
    hist[k] = fetch(d_out[k], sz);
    sz = cap;
    st = m.compress(d_in, n, d_out[k], &sz, d_temp, ts, in.data() + 5000, 4096, 0);
    REQ(st == Status::SUCCESS, "compress with a dictionary (ldm %d): %s", k, status_to_string(st));
    dict[k] = fetch(d_out[k], sz);
    CK(hipFree(d_temp));
  }
  REQ(hist[0] == hist[1], "compress_with_history depends on the flag");
  REQ(dict[0] == dict[1], "compress() with a dictionary depends on the flag");
  REQ(hist[0] != plain[0] && dict[0] != plain[0], "history / dictionary frames equal the plain frame");
  printf("ldm paths OK: compress %zu -> %zu with the flag\n", plain[0].size(), plain[1].size());
  return 0;
}

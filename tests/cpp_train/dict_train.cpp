// dict_train.cpp — the C++ training entries with device samples, driven by
// tests/test_gpu_dict_train.py (-m gpu).  Built by __graft_entry__.build() (tests/cpp_train/Makefile)
// against libcuda_zstd_hip.so; test infrastructure only.
//
//   dict_train <dir> <dict_size>
// <dir>/in.bin = the samples back to back, <dir>/sizes.bin = u64 sizes.  Calls
// dictionary::train_dictionary with host pointers (the expected bytes), then with device pointers
// into one buffer (trained in place), with separately allocated device samples (gathered), with
// use_gpu = false on device pointers, and into a device dict_buffer; then
// create_dictionary_from_samples with a host and with a device buffer (device dict_buffer).
// Exits non-zero unless every buffer equals its host counterpart; writes <dir>/dict.bin.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "cuda_zstd_dictionary.h"

using namespace cuda_zstd;

#define CK(x)                                                                  \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess) {                                                    \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      return 2;                                                                \
    }                                                                          \
  } while (0)
#define WANT(cond)                                            \
  do {                                                        \
    if (!(cond)) {                                            \
      fprintf(stderr, "%s:%d failed: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                               \
    }                                                         \
  } while (0)

static std::vector<unsigned char> slurp(const std::string &p) {
  std::ifstream f(p, std::ios::binary);
  return std::vector<unsigned char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
  if (argc < 3) return 64;
  std::string const dir = argv[1];
  size_t const dict_size = (size_t)atoll(argv[2]);
  std::vector<unsigned char> in = slurp(dir + "/in.bin"), sz = slurp(dir + "/sizes.bin");
  size_t const n = sz.size() / 8;
  WANT(n > 0 && !in.empty());
  std::vector<size_t> sizes(n), offs(n);
  size_t total = 0;
  for (size_t i = 0; i < n; i++) {
    unsigned long long v;
    memcpy(&v, sz.data() + 8 * i, 8);
    sizes[i] = (size_t)v;
    offs[i] = total;
    total += sizes[i];
  }
  WANT(total == in.size());

  // expected: host pointers
  std::vector<const void *> hp(n);
  for (size_t i = 0; i < n; i++) hp[i] = in.data() + offs[i];
  std::vector<unsigned char> want(dict_size), got(dict_size);
  WANT(dictionary::train_dictionary(hp, sizes, want.data(), dict_size) == Status::SUCCESS);

  hipStream_t stream;
  CK(hipStreamCreate(&stream));
  // one device buffer: trained in place
  unsigned char *d_all = nullptr;
  CK(hipMalloc((void **)&d_all, total + 8192));
  CK(hipMemset(d_all, 0, total + 8192));
  CK(hipMemcpy(d_all, in.data(), total, hipMemcpyHostToDevice));
  std::vector<const void *> dp(n);
  for (size_t i = 0; i < n; i++) dp[i] = d_all + offs[i];
  got.assign(dict_size, 0xEE);
  WANT(dictionary::train_dictionary(dp, sizes, got.data(), dict_size, nullptr, stream) == Status::SUCCESS);
  WANT(got == want);

  // separately allocated samples: gathered
  std::vector<void *> owned(n, nullptr);
  std::vector<const void *> sp(n);
  for (size_t i = 0; i < n; i++) {
    CK(hipMalloc(&owned[i], sizes[i] ? sizes[i] : 1));
    if (sizes[i]) CK(hipMemcpy(owned[i], in.data() + offs[i], sizes[i], hipMemcpyHostToDevice));
    sp[i] = owned[i];
  }
  dictionary::DictionaryTrainingParams on;
  got.assign(dict_size, 0xEE);
  WANT(dictionary::train_dictionary(sp, sizes, got.data(), dict_size, &on, stream) == Status::SUCCESS);
  WANT(got == want);

  // use_gpu = false with device pointers: copied out and trained on the host
  dictionary::DictionaryTrainingParams off;
  off.use_gpu = false;
  got.assign(dict_size, 0xEE);
  WANT(dictionary::train_dictionary(sp, sizes, got.data(), dict_size, &off, stream) == Status::SUCCESS);
  WANT(got == want);
  // host pointers ignore use_gpu
  got.assign(dict_size, 0xEE);
  WANT(dictionary::train_dictionary(hp, sizes, got.data(), dict_size, &on) == Status::SUCCESS);
  WANT(got == want);

  // a device dict_buffer
  unsigned char *d_dict = nullptr;
  CK(hipMalloc((void **)&d_dict, dict_size));
  CK(hipMemset(d_dict, 0xEE, dict_size));
  WANT(dictionary::train_dictionary(dp, sizes, d_dict, dict_size, nullptr, stream) == Status::SUCCESS);
  CK(hipMemcpy(got.data(), d_dict, dict_size, hipMemcpyDeviceToHost));
  WANT(got == want);

  // create_dictionary_from_samples: the last sample runs 8 KiB from its offset
  std::vector<unsigned char> padded(in);
  padded.resize(total + 8192, 0);
  std::vector<unsigned char> want2(dict_size);
  WANT(dictionary::create_dictionary_from_samples(padded.data(), offs.data(), n, want2.data(), dict_size) == Status::SUCCESS);
  CK(hipMemset(d_dict, 0xEE, dict_size));
  WANT(dictionary::create_dictionary_from_samples(d_all, offs.data(), n, d_dict, dict_size, nullptr, stream) == Status::SUCCESS);
  got.assign(dict_size, 0xEE);
  CK(hipMemcpy(got.data(), d_dict, dict_size, hipMemcpyDeviceToHost));
  WANT(got == want2);

  // argument checks are unchanged for device samples
  WANT(dictionary::train_dictionary(dp, sizes, got.data(), 100, nullptr, stream) == Status::ERROR_INVALID_PARAMETER);

  std::ofstream(dir + "/dict.bin", std::ios::binary).write((const char *)want.data(), (std::streamsize)want.size());
  for (void *p : owned) CK(hipFree(p));
  CK(hipFree(d_dict));
  CK(hipFree(d_all));
  CK(hipStreamDestroy(stream));
  printf("dict_train OK: %zu samples, %zu bytes\n", n, total);
  return 0;
}

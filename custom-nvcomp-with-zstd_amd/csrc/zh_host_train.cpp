// zh_host_train.cpp — host runtime, dictionary training and finalize, with their C entries.
#include "zh_dict.h"
#include "zh_dict_finalize.h"
#include "zh_dict_train.h"
#include "zh_host.h"

namespace cuda_zstd {
// dictionary training API (reference include/cuda_zstd_dictionary.h:176-210,
// src/cuda_zstd_dictionary.cu:421-520): COVER (zh_dict.cpp) instead of the reference's
// byte-frequency / 4-gram fill, same validation and buffer contract
namespace dictionary {
namespace {
bool g_train_profile = false;  // cuda_zstd_hip_dict_train_profile: HIP events around the device trainer's kernel groups
float g_train_phase_ms[3] = {0.f, 0.f, 0.f};

// the groups' sample counts add up to the n samples
bool groups_cover(const size_t *counts, size_t ng, size_t n) {
  size_t counted = 0, g = 0;
  for (; g < ng && counts[g] <= n - counted; g++) counted += counts[g];
  return g == ng && counted == n;
}
}  // namespace

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
  if (!groups_cover(counts, ng, n)) return Status::ERROR_INVALID_PARAMETER;
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

namespace {
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
      if (on_gpu) {  // samples that are not back to back are gathered first
        u8 *gathered = nullptr;
        if (!contiguous && hipMalloc((void **)&gathered, total) != hipSuccess) { (void)hipGetLastError(); return Status::ERROR_OUT_OF_MEMORY; }
        size_t o = 0;
        hipError_t e = hipSuccess;
        for (auto const &p : s) {
          if (gathered && p.second && e == hipSuccess) e = hipMemcpyAsync(gathered + o, p.first, p.second, hipMemcpyDeviceToDevice, stream);
          o += p.second;
        }
        Status st = e == hipSuccess ? Status::SUCCESS : Status::ERROR_CUDA_ERROR;
        if (st == Status::SUCCESS)
          st = train_device(gathered ? gathered : (const u8 *)first, sample_sizes.data(), samples.size(), dict_size, 0, 0, nullptr, 0, true, stream, c);
        else (void)hipStreamSynchronize(stream);
        if (gathered) (void)hipFree(gathered);
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

}  // namespace cuda_zstd

using namespace cuda_zstd;
using nvcomp_v5::status_to_nvcomp_error;

extern "C" {
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
size_t cuda_zstd_train_dictionaries_device_get_temp_size(const size_t *sizes, size_t num, const size_t *counts, size_t num_groups, size_t dict_size,
                                                         unsigned k) {
  if (!sizes || !counts || num_groups == 0 || num_groups > zh::kCoverMaxGroups) return 0;
  return dictionary::groups_cover(counts, num_groups, num) ? zh::cover_temp_bytes(sizes, num, counts, num_groups, dict_size, k) : 0;
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
// one dictionary from all samples: the call with one group (no dictionary from it: ERROR_COMPRESSION, where the host entry returns NULL)
int cuda_zstd_train_dictionary_device(const void *d_samples, const size_t *sizes, size_t num, size_t dict_size, unsigned k, unsigned d,
                                      void *d_temp, size_t temp_bytes, hipStream_t stream, cuda_zstd_dict_t **dict_out) {
  if (!dict_out) return c_err(Status::ERROR_INVALID_PARAMETER);
  int const rc = cuda_zstd_train_dictionaries_device(d_samples, sizes, num, &num, 1, dict_size, k, d, d_temp, temp_bytes, stream, dict_out, nullptr);
  return rc || *dict_out ? rc : c_err(Status::ERROR_COMPRESSION);
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

}  // extern "C"

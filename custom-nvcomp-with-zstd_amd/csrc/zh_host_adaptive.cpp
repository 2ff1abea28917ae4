// zh_host_adaptive.cpp — host runtime, adaptive level selection with its C entries.
#include "zh_adaptive.h"
#include "zh_host.h"

namespace cuda_zstd {
// adaptive level selection (include/cuda_zstd_adaptive.h; reference src/cuda_zstd_adaptive.cu)
// One device buffer through the batch kernels (zh_adaptive.hip): the record, the statistics and
// the level live in one small allocation; one copy back, one wait.
Status adaptive_one(const void *d_data, size_t size, size_t sample_bytes, int preference, cuda_zstd_adaptive_stats_t &out, hipStream_t stream) {
  if (!d_data || size == 0 || sample_bytes == 0 || preference < 0 || preference > 2) return Status::ERROR_INVALID_PARAMETER;
  size_t const rec = ZH_AD_REC_WORDS * sizeof(u32);
  u8 *d = nullptr;
  if (hipMalloc((void **)&d, rec + sizeof(out) + sizeof(int)) != hipSuccess) { (void)hipGetLastError(); return Status::ERROR_OUT_OF_MEMORY; }
  auto *const d_stats = (cuda_zstd_adaptive_stats_t *)(d + rec);
  bool const ok = zh::adaptive_launch(nullptr, nullptr, d_data, size, 1, std::min(sample_bytes, size), preference, d_stats,
                                      (int *)(d + rec + sizeof(out)), (u32 *)d, stream) == hipSuccess &&
                  hipMemcpyAsync(&out, d_stats, sizeof(out), hipMemcpyDeviceToHost, stream) == hipSuccess &&
                  hipStreamSynchronize(stream) == hipSuccess;
  (void)hipFree(d);
  if (!ok) { (void)hipGetLastError(); return Status::ERROR_CUDA_ERROR; }
  return Status::SUCCESS;
}

namespace {
// The branch of the rule behind a result (the level table's rows differ, except RANDOM / LOW)
int adaptive_branch(const cuda_zstd_adaptive_stats_t &s, int preference) {
  if (!s.sample_size) return ZH_AD_EMPTY;
  if (s.flags & ZH_AD_IS_RANDOM) return ZH_AD_RANDOM;
  for (int b = ZH_AD_REPETITIVE; b < ZH_AD_LOW; b++)
    if (zh_adaptive_level(b, preference) == s.level) return b;
  return ZH_AD_LOW;
}
const char *const kAdaptiveReasoning[ZH_AD_BRANCHES] = {
    "high entropy and no short-period patterns: the data looks random, a fast level loses nothing",
    "long runs or mostly repeated bytes: a deep search is cheap here and pays",
    "low entropy with many repeated bytes: highly compressible, a strong level pays",
    "moderately compressible: a middle level",
    "little redundancy in the byte statistics: a fast level",
    "empty input: the default level",
};
}  // namespace

namespace adaptive {

AdaptiveLevelSelector::AdaptiveLevelSelector() = default;
AdaptiveLevelSelector::AdaptiveLevelSelector(AdaptivePreference pref) : preference_(pref) {}
AdaptiveLevelSelector::~AdaptiveLevelSelector() = default;
void AdaptiveLevelSelector::set_preference(AdaptivePreference pref) { preference_ = pref; }
void AdaptiveLevelSelector::set_sample_size(size_t size) { sample_size_ = size; }
void AdaptiveLevelSelector::enable_quick_analysis(bool enable) { quick_mode_ = enable; }  // (never read: see the header)
const DataCharacteristics &AdaptiveLevelSelector::get_last_characteristics() const { return last_characteristics_; }
void AdaptiveLevelSelector::reset_statistics() { last_characteristics_ = DataCharacteristics(); }

Status AdaptiveLevelSelector::select_level(const void *d_data, size_t data_size, AdaptiveResult &result, hipStream_t stream) {
  cuda_zstd_adaptive_stats_t s;
  Status const st = adaptive_one(d_data, data_size, sample_size_, (int)preference_, s, stream);
  if (st != Status::SUCCESS) return ZH_NOTED(st);
  DataCharacteristics &c = last_characteristics_;
  c.entropy = s.entropy;
  c.repetition_ratio = s.repetition_ratio;
  c.compressibility = s.compressibility;
  c.unique_bytes = s.unique_bytes;
  c.max_run_length = s.max_run_length;
  c.avg_match_length = 0;
  c.has_patterns = (s.flags & ZH_AD_HAS_PATTERNS) != 0;
  c.is_random = (s.flags & ZH_AD_IS_RANDOM) != 0;
  result.recommended_level = s.level;
  result.recommended_strategy = CompressionConfig::level_to_strategy(s.level);
  result.characteristics = c;
  result.confidence = 0.85f;
  result.reasoning = kAdaptiveReasoning[adaptive_branch(s, (int)preference_)];
  return Status::SUCCESS;
}

Status select_adaptive_level(const void *d_data, size_t data_size, int &recommended_level, AdaptivePreference preference, hipStream_t stream) {
  AdaptiveResult r;
  Status const st = AdaptiveLevelSelector(preference).select_level(d_data, data_size, r, stream);
  if (st == Status::SUCCESS) recommended_level = r.recommended_level;
  return st;
}
Status analyze_and_select(const void *d_data, size_t data_size, AdaptiveResult &result, AdaptivePreference preference, hipStream_t stream) {
  return AdaptiveLevelSelector(preference).select_level(d_data, data_size, result, stream);
}
Status is_compressible(const void *d_data, size_t data_size, bool &compressible, float &estimated_ratio, hipStream_t stream) {
  AdaptiveResult r;
  Status const st = AdaptiveLevelSelector(AdaptivePreference::BALANCED).select_level(d_data, data_size, r, stream);
  if (st != Status::SUCCESS) return st;
  compressible = r.characteristics.compressibility > 0.3f;
  estimated_ratio = 1.0f + r.characteristics.compressibility * 3.0f;
  return Status::SUCCESS;
}

}  // namespace adaptive

}  // namespace cuda_zstd

using namespace cuda_zstd;

extern "C" {
// ---- adaptive level selection (zh_adaptive.hip; the rule in zh_adaptive.h) ---------------------
size_t cuda_zstd_adaptive_get_temp_size(size_t num_chunks) { return num_chunks * ZH_AD_REC_WORDS * sizeof(u32); }

int cuda_zstd_adaptive_analyze_batch_async(const void *const *d_ptrs, const size_t *d_sizes, size_t num_chunks, size_t sample_bytes,
                                           int preference, cuda_zstd_adaptive_stats_t *d_stats, int *d_levels, void *d_temp,
                                           size_t temp_bytes, hipStream_t stream) {
  if (preference < 0 || preference > 2 || sample_bytes == 0) return c_err(Status::ERROR_INVALID_PARAMETER);
  if (num_chunks == 0) return 0;
  if (!d_ptrs || !d_sizes || !d_levels || !d_temp || ((uintptr_t)d_temp & 3u) || !zh::adaptive_grid(num_chunks, sample_bytes))
    return c_err(Status::ERROR_INVALID_PARAMETER);
  if (temp_bytes < cuda_zstd_adaptive_get_temp_size(num_chunks)) return c_err(Status::ERROR_BUFFER_TOO_SMALL);
  hipError_t const e = zh::adaptive_launch(d_ptrs, d_sizes, nullptr, 0, num_chunks, sample_bytes, preference, d_stats, d_levels, (u32 *)d_temp, stream);
  return e == hipSuccess ? 0 : c_err(Status::ERROR_CUDA_ERROR);
}

int cuda_zstd_adaptive_select_level(const void *d_data, size_t size, size_t sample_bytes, int preference, cuda_zstd_adaptive_stats_t *h_out,
                                    hipStream_t stream) {
  if (!h_out) return c_err(Status::ERROR_INVALID_PARAMETER);
  return c_err(adaptive_one(d_data, size, sample_bytes, preference, *h_out, stream));
}

int cuda_zstd_adaptive_finalize_host(const unsigned *hist256, unsigned sample_size, unsigned repeated_pairs, unsigned max_run_length,
                                     unsigned pattern_score, int preference, cuda_zstd_adaptive_stats_t *out) {
  if (!hist256 || !out || preference < 0 || preference > 2) return c_err(Status::ERROR_INVALID_PARAMETER);
  float const inv_n = sample_size ? 1.0f / (float)sample_size : 0.0f;
  float ent = 0.0f;
  u32 uniq = 0;
  for (u32 i = 0; i < 256; i++) {
    uniq += hist256[i] != 0;
    ent += zh_adaptive_entropy_term(hist256[i], inv_n);
  }
  zh_adaptive_decide(sample_size, repeated_pairs, max_run_length, pattern_score, uniq, ent, preference, out);
  return 0;
}

}  // extern "C"

// cuda_zstd_adaptive.h — adaptive compression-level selection of the gfx950 Zstandard compressor.
//
// Drop-in counterpart of the reference's include/cuda_zstd_adaptive.h (same names, fields,
// defaults and semantics, cudaStream_t -> hipStream_t, so a reference caller compiles unchanged):
//   AdaptivePreference, DataCharacteristics, AdaptiveResult      :18-41
//   AdaptiveLevelSelector (public methods)                       :47-68
//   select_adaptive_level / analyze_and_select / is_compressible :93-117
//
// The level rule is the reference's decision tree (src/cuda_zstd_adaptive.cu), so the same data
// gets the same level.  What differs: the statistics of a buffer come from one stream-ordered
// launch (csrc/zh_adaptive.hip) instead of four kernels with their own allocations and blocking
// copies; unique_bytes is filled in (the reference leaves it 0); buffers shorter than 5 bytes
// have pattern score 0 (the reference's unsigned size - 4 wraps there).  Whole batches are
// analysed, results left on the device, by cuda_zstd_adaptive_analyze_batch_async
// (cuda_zstd_capi.h).
#ifndef CUDA_ZSTD_ADAPTIVE_H_
#define CUDA_ZSTD_ADAPTIVE_H_

#include "cuda_zstd_types.h"

namespace cuda_zstd {
namespace adaptive {

enum class AdaptivePreference { SPEED = 0, BALANCED = 1, RATIO = 2 };

struct DataCharacteristics {
  float entropy = 0.0f;           // Shannon entropy of the sample's bytes, 0..8 bits
  float repetition_ratio = 0.0f;  // positions whose next byte is equal, over the sample size
  float compressibility = 0.0f;   // 0..1 estimate from entropy and repetition
  u32 unique_bytes = 0;           // distinct byte values in the sample
  u32 max_run_length = 0;         // longest run of equal bytes, saturating at 256
  u32 avg_match_length = 0;       // never computed (0), as in the reference
  bool has_patterns = false;      // short-period repeats are frequent
  bool is_random = false;         // entropy above 7.5 bits and no patterns
};

struct AdaptiveResult {
  int recommended_level = 3;
  Strategy recommended_strategy = Strategy::GREEDY;
  DataCharacteristics characteristics;
  float confidence = 0.0f;
  const char *reasoning = nullptr;  // static string naming the branch of the rule
};

class AdaptiveLevelSelector {
 public:
  AdaptiveLevelSelector();
  explicit AdaptiveLevelSelector(AdaptivePreference pref);
  ~AdaptiveLevelSelector();

  // Analyses the first min(data_size, sample size) bytes of a device buffer on `stream` and waits
  // for the result.  ERROR_INVALID_PARAMETER for a null pointer or data_size 0.
  Status select_level(const void *d_data, size_t data_size, AdaptiveResult &result, hipStream_t stream = 0);

  void set_preference(AdaptivePreference pref);
  void set_sample_size(size_t size);  // bytes analysed from the front of the buffer (default 64 KiB)
  // Stored and without effect, as in the reference (which never reads the flag): there is one
  // analysis, and it is a single pass.
  void enable_quick_analysis(bool enable);

  const DataCharacteristics &get_last_characteristics() const;
  void reset_statistics();

 private:
  AdaptivePreference preference_ = AdaptivePreference::BALANCED;
  size_t sample_size_ = 64 * 1024;
  bool quick_mode_ = false;
  DataCharacteristics last_characteristics_;
};

// The level alone.
Status select_adaptive_level(const void *d_data, size_t data_size, int &recommended_level,
                             AdaptivePreference preference = AdaptivePreference::BALANCED, hipStream_t stream = 0);
// Level, strategy, characteristics and reasoning.
Status analyze_and_select(const void *d_data, size_t data_size, AdaptiveResult &result,
                          AdaptivePreference preference = AdaptivePreference::BALANCED, hipStream_t stream = 0);
// compressible = compressibility > 0.3; estimated_ratio = 1 + 3 * compressibility.
Status is_compressible(const void *d_data, size_t data_size, bool &compressible, float &estimated_ratio, hipStream_t stream = 0);

}  // namespace adaptive
}  // namespace cuda_zstd

#endif  // CUDA_ZSTD_ADAPTIVE_H_

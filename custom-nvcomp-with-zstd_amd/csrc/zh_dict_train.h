// zh_dict_train.h — COVER training on the device (zh_dict_train.hip; geometry: zh_dict_plan.h).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "zh_dict_plan.h"

namespace zh {
// Trains on the ns samples lying back to back at d_corpus (ends: HOST prefix sums of their sizes,
// ends[ns - 1] = plan.N < 2^32 - 64) and leaves in `out` the bytes zh::cover_train returns for the
// same samples.  plan = cover_plan(N, dict_size, k, d), not empty, k <= kCoverMaxK; temp: at least
// cover_temp_layout(plan, ns, dict_size).total bytes of device memory.  Reads of d_corpus are
// ordered on `stream`; the call returns after the stream has drained.
// phase_ms (optional, 3 floats): device time of ids + freq, prevdist, the step loop.
hipError_t cover_train_device(const uint8_t *d_corpus, const uint32_t *ends, size_t ns, const CoverPlan &plan, size_t dict_size,
                              void *temp, hipStream_t stream, std::vector<uint8_t> &out, float *phase_ms = nullptr);
}  // namespace zh

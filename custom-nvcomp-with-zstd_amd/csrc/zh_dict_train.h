// zh_dict_train.h — COVER training on the device (zh_dict_train.hip; geometry: zh_dict_plan.h).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "zh_dict_plan.h"

namespace zh {
// Trains one dictionary per group on the ns samples lying back to back at d_corpus (ends: HOST
// prefix sums of their sizes, ends[ns - 1] < 2^32 - 64; groups: the HOST records cover_groups made
// of the same sizes, 1 <= ng <= kCoverMaxGroups, k <= kCoverMaxK) and leaves in out[g] the bytes
// zh::cover_train returns for group g's samples alone (none for a group whose plan is empty).
// temp: at least cover_temp_layout(bytes, ns, ng, the groups' largest ntiles, dict_size).total bytes
// of device memory.  Reads of d_corpus are ordered on `stream`; the call returns after the stream
// has drained.  Groups run in waves of kCoverGroupsInFlight; the launches of a wave do not depend
// on how many groups it holds.
// phase_ms (optional, 3 floats): device time of ids + freq, prevdist, the step loops, over all waves.
hipError_t cover_train_groups_device(const uint8_t *d_corpus, const uint32_t *ends, size_t ns, const CoverGroup *groups, size_t ng,
                                     size_t dict_size, void *temp, hipStream_t stream, std::vector<std::vector<uint8_t>> &out,
                                     float *phase_ms = nullptr);
}  // namespace zh

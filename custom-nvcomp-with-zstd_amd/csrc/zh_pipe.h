// zh_pipe.h — the decoder's side stream (host code).
//
// The split pipeline of zh_decode.hip (launch_decompress) runs one kernel beside the caller's
// stream: an event orders the side stream after the tables pass, a second one orders the
// execution after the side stream's kernel.  One set per device, created on the device of the
// caller's stream at its first large call and kept; a call holds the set's mutex while it
// enqueues its kernels.
#ifndef ZH_PIPE_H_
#define ZH_PIPE_H_

#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <mutex>

namespace zh {

struct SidePipe {
  std::mutex mu;
  hipStream_t side = nullptr;
  hipEvent_t tables_done = nullptr, rest_done = nullptr;
  bool ok = true;
  explicit SidePipe(int dev) {
    int cur = -1;
    ok = hipGetDevice(&cur) == hipSuccess && hipSetDevice(dev) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&side, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&tables_done, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&rest_done, hipEventDisableTiming) == hipSuccess;
    if (cur >= 0) (void)hipSetDevice(cur);
  }
};

// The device a stream belongs to (the null stream: the current device)
inline int stream_device(hipStream_t s) {
  int dev = -1;
  if (s && hipStreamGetDevice(s, &dev) == hipSuccess) return dev;
  (void)hipGetLastError();
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  return dev;
}

// The side pipe of the device of s; null if its stream or events could not be created
inline SidePipe *side_pipe(hipStream_t s) {
  static std::mutex mu;
  static std::map<int, std::unique_ptr<SidePipe>> pipes;
  int const dev = stream_device(s);
  std::lock_guard<std::mutex> lk(mu);
  auto &p = pipes[dev];
  if (!p) p.reset(new SidePipe(dev));
  return p->ok ? p.get() : nullptr;
}

}  // namespace zh
#endif  // ZH_PIPE_H_

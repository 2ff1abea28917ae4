// zh_stream.hip — many streams in one call (cuda_zstd_stream_batch_*, zh_host.cpp): the windows of
// all streams advance on the device.
//
// zh_window_update_kernel: one workgroup per stream.  Stream i's window is a pair of
//   ZH_STREAM_WINDOW-byte buffers; the current one holds the stream's last pre_sizes[i] bytes and is
//   what pre_ptrs[i] points to (the prefix the batch entries compress or decode the next chunk
//   behind).  After a call the kernel writes the last <= ZH_STREAM_WINDOW bytes of window ++ chunk
//   into the other buffer and makes it the current one.  A stream whose item did not succeed (status
//   non-zero, or no bytes) keeps its window.  The index arithmetic is zh_stream_window.h's; the
//   kernel only moves bytes.
// zh_window_reset_kernel: every stream back to an empty window.
#include "zh_common.h"
#include "zh_launch.h"
#include "zh_stream_window.h"

#include <mutex>
#include <vector>

#define ZH_WIN_THREADS 256u

// 16 bytes from any address (the compiler picks the widest load the target allows unaligned)
typedef u32 zh_v4u __attribute__((ext_vector_type(4)));
typedef zh_v4u zh_v4u_any __attribute__((aligned(1)));

// n bytes from src to dst, the whole workgroup: byte stores up to dst's first 16-byte boundary,
// 16-byte stores over the aligned middle (loads at whatever alignment src has there), bytes at the end
__device__ __forceinline__ void wg_copy(u8 *__restrict__ dst, const u8 *__restrict__ src, u64 n) {
  u32 const tid = threadIdx.x;
  ZhCopySplit const s = zh_copy_split((uintptr_t)dst, n);
  if (tid < s.head) dst[tid] = src[tid];
  u8 *const dm = dst + s.head;
  const u8 *const sm = src + s.head;
  for (u64 v = tid; v < s.vec; v += ZH_WIN_THREADS) {
    zh_v4u const q = *(const zh_v4u_any *)(sm + 16u * v);
    *(zh_v4u *)(dm + 16u * v) = q;
  }
  u64 const t0 = s.head + 16u * s.vec;
  if (tid < s.tail) dst[t0 + tid] = src[t0 + tid];
}

extern "C" __global__ __launch_bounds__(ZH_WIN_THREADS) void zh_window_update_kernel(u8 *__restrict__ windows, u32 *__restrict__ which,
                                                                                      const void **pre_ptrs, size_t *pre_sizes,
                                                                                      const void *const *__restrict__ chunk_ptrs,
                                                                                      const size_t *__restrict__ chunk_sizes,
                                                                                      const u32 *__restrict__ statuses) {
  u32 const i = blockIdx.x;
  u64 const n = chunk_sizes[i];
  if (statuses[i] != 0 || n == 0) return;  // failed or idle: the window stays
  u32 const cur = which[i] & 1u;
  u64 const len = pre_sizes[i];
  u8 *const pair = windows + (size_t)i * 2u * ZH_STREAM_WINDOW;
  const u8 *const old = pair + (size_t)cur * ZH_STREAM_WINDOW;
  u8 *const next = pair + (size_t)(cur ^ 1u) * ZH_STREAM_WINDOW;
  ZhWindowMove const m = zh_window_move(len, n, ZH_STREAM_WINDOW);
  wg_copy(next, old + m.keep_from, m.keep);
  wg_copy(next + m.keep, (const u8 *)chunk_ptrs[i] + m.take_from, m.take);
  __syncthreads();  // every thread has read which[i] and pre_sizes[i]
  if (threadIdx.x == 0) {
    which[i] = cur ^ 1u;
    pre_ptrs[i] = next;
    pre_sizes[i] = (size_t)(m.keep + m.take);
  }
}

extern "C" __global__ void zh_window_reset_kernel(u8 *windows, u32 *which, const void **pre_ptrs, size_t *pre_sizes, u32 nstreams) {
  u32 const i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nstreams) return;
  which[i] = 0;
  pre_ptrs[i] = windows + (size_t)i * 2u * ZH_STREAM_WINDOW;
  pre_sizes[i] = 0;
}

namespace zh {

namespace {
struct WinProf {
  std::mutex mu;
  bool on = false;
  std::vector<hipEvent_t> ev;  // pairs around each window launch
};
WinProf &win_prof() {
  static WinProf p;
  return p;
}
}  // namespace

// HIP events around zh_window_update_kernel (tools/prefix_batch_bench.py).  off: returns the summed
// milliseconds of the launches recorded since it was switched on
double window_profile(bool on) {
  WinProf &p = win_prof();
  std::lock_guard<std::mutex> g(p.mu);
  double ms = 0;
  for (size_t i = 0; i + 1 < p.ev.size(); i += 2) {
    float t = 0;
    (void)hipEventSynchronize(p.ev[i + 1]);
    (void)hipEventElapsedTime(&t, p.ev[i], p.ev[i + 1]);
    ms += t;
    (void)hipEventDestroy(p.ev[i]);
    (void)hipEventDestroy(p.ev[i + 1]);
  }
  p.ev.clear();
  p.on = on;
  return ms;
}

hipError_t window_update_launch(u8 *windows, u32 *which, const void **pre_ptrs, size_t *pre_sizes, const void *const *chunk_ptrs,
                                const size_t *chunk_sizes, const u32 *statuses, u32 nstreams, hipStream_t stream) {
  if (!nstreams) return hipSuccess;
  bool prof;
  {
    std::lock_guard<std::mutex> g(win_prof().mu);
    prof = win_prof().on;
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;  // (profiling only: a call otherwise creates nothing)
  if (prof && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) {
    if (e0) (void)hipEventDestroy(e0);
    e0 = e1 = nullptr;
  }
  if (e0) (void)hipEventRecord(e0, stream);
  hipLaunchKernelGGL(zh_window_update_kernel, dim3(nstreams), dim3(ZH_WIN_THREADS), 0, stream, windows, which, pre_ptrs, pre_sizes, chunk_ptrs,
                     chunk_sizes, statuses);
  if (e0) {
    (void)hipEventRecord(e1, stream);
    std::lock_guard<std::mutex> g(win_prof().mu);
    win_prof().ev.push_back(e0);
    win_prof().ev.push_back(e1);
  }
  return hipGetLastError();
}
hipError_t window_reset_launch(u8 *windows, u32 *which, const void **pre_ptrs, size_t *pre_sizes, u32 nstreams, hipStream_t stream) {
  if (!nstreams) return hipSuccess;
  hipLaunchKernelGGL(zh_window_reset_kernel, dim3((nstreams + 255) / 256), dim3(256), 0, stream, windows, which, pre_ptrs, pre_sizes, nstreams);
  return hipGetLastError();
}
}  // namespace zh

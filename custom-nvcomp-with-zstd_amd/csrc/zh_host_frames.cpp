// zh_host_frames.cpp — host runtime, the frame-index driver (C entries): the seek table of a
// buffer of concatenated frames (zh_frames.hip).
#include "zh_frames_index.h"
#include "zh_host.h"

#include <atomic>

using namespace cuda_zstd;

using nvcomp_v5::status_to_nvcomp_error;
static int const kFramesInvalid = status_to_nvcomp_error(Status::ERROR_INVALID_PARAMETER),
                 kFramesDevice = status_to_nvcomp_error(Status::ERROR_CUDA_ERROR),
                 kFramesTooSmall = status_to_nvcomp_error(Status::ERROR_BUFFER_TOO_SMALL);

// Test and benchmark hooks: the path (0 auto, 1 the serial walker), and the last call's split
static std::atomic<int> g_frames_path{0};
static std::atomic<int> g_frames_last_path{-1};
static std::atomic<int> g_frames_split_on{0};
static float g_frames_split[4];  // ms of the write, span, reach and collect kernels
static std::mutex g_frames_split_mutex;

static bool read_ctl(zh::FramesCtl &ctl, const u8 *base, hipStream_t stream) {
  return hipMemcpyAsync(&ctl, base, sizeof(ctl), hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
}

extern "C" {

void cuda_zstd_hip_frames_index_path(int path) { g_frames_path = path; }
// The path the last call that launched anything took: 0 the speculative index, 1 the serial walker (-1: none yet)
int cuda_zstd_hip_frames_index_last_path(void) { return g_frames_last_path; }

// Benchmark hook: on != 0 makes every auto-path call time its kernels with events; ms (4 floats,
// may be null) receives the last such call's write, span, reach and collect times.
void cuda_zstd_hip_frames_index_split(int on, float *ms) {
  g_frames_split_on = on;
  std::lock_guard<std::mutex> lock(g_frames_split_mutex);
  if (ms) std::copy(g_frames_split, g_frames_split + 4, ms);
}

size_t cuda_zstd_seekable_index_get_temp_size(size_t stream_bytes, size_t max_frames) {
  if (stream_bytes == 0) return 0;  // (the call answers an empty stream with 2)
  return zh::frames_temp_bytes(stream_bytes, (size_t)std::min<u64>(max_frames, ZH_SEEK_MAX_FRAMES));
}

int cuda_zstd_seekable_index(nvcomp_zstd_batch_manager_t *mgr, const void *d_stream, size_t size, size_t max_frames, void *d_table,
                             size_t table_capacity, size_t *table_bytes, size_t *num_frames, unsigned long long *error_offset, void *d_temp,
                             size_t temp_bytes, hipStream_t stream) {
  if (table_bytes) *table_bytes = 0;
  if (num_frames) *num_frames = 0;
  if (error_offset) *error_offset = 0;
  if ((mgr && !mgr->mgr) || !d_stream || !size || !d_table || !table_bytes || !num_frames || !error_offset)
    return c_err(Status::ERROR_INVALID_PARAMETER);
  size_t const n = (size_t)std::min<u64>(max_frames, ZH_SEEK_MAX_FRAMES);
  if (!d_temp || temp_bytes < zh::frames_temp_bytes(size, n)) return kFramesTooSmall;  // nothing launched
  if (ensure_kernels() != Status::SUCCESS) return kFramesDevice;
  u8 *const base = aligned_base(d_temp);
  zh::FramesCtl ctl;

  // ---- the frames: entries and size jobs in the temp buffer, the stream's verdict
  bool serial = g_frames_path == 1;
  if (!serial) {
    if (zh::frames_count_launch(d_stream, size, n, base, stream) != hipSuccess || !read_ctl(ctl, base, stream)) return kFramesDevice;
    serial = ctl.ncand > ZH_FRAMES_CANDIDATES(n);
  }
  g_frames_last_path = serial ? 1 : 0;
  if (serial) {
    // (the count kernels may have run; the control block starts over)
    if (hipMemsetAsync(base, 0, sizeof(ctl), stream) != hipSuccess ||
        hipMemsetAsync(base + offsetof(zh::FramesCtl, errkey), 0xFF, 16, stream) != hipSuccess ||
        zh::frames_walk_launch(d_stream, size, n, base, stream) != hipSuccess)
      return kFramesDevice;
  } else {
    bool const timed = g_frames_split_on != 0;
    hipEvent_t ev[5] = {};
    if (timed)
      for (auto &e : ev)
        if (hipEventCreate(&e) != hipSuccess) return kFramesDevice;
    hipError_t const e = zh::frames_reach_launch(d_stream, size, n, (size_t)ctl.ncand, base, timed ? ev : nullptr, stream);
    if (timed) {
      (void)hipStreamSynchronize(stream);
      std::lock_guard<std::mutex> lock(g_frames_split_mutex);
      for (int i = 0; i < 4; i++)
        if (hipEventElapsedTime(&g_frames_split[i], ev[i], ev[i + 1]) != hipSuccess) g_frames_split[i] = -1.f;
      for (auto &x : ev) (void)hipEventDestroy(x);
    }
    if (e != hipSuccess) return kFramesDevice;
  }
  if (!read_ctl(ctl, base, stream)) return kFramesDevice;
  *num_frames = (size_t)ctl.nframes;
  if (ctl.status != ZH_FRAMES_OK) {  // malformed: the frames before the failing one, and its offset
    *error_offset = ctl.err_off;
    return (int)zh_frames_code(ctl.status);
  }
  // (max_frames too small: *num_frames tells the caller what the stream needs)
  if (ctl.nframes > n) return ctl.nframes > ZH_SEEK_MAX_FRAMES ? kFramesInvalid : kFramesTooSmall;
  if (ctl.limit) return kFramesInvalid;
  size_t const table = (size_t)zh_seek_table_bytes(ctl.nframes, 0);
  if (table_capacity < table) return kFramesTooSmall;

  // ---- the frames without a Frame_Content_Size: the decoder's size pass, with the handle's dictionaries
  if (ctl.njobs) {
    zh::FramesJobs const j = zh::frames_jobs(base, size, n);
    if (mgr) {
      Status const s = mgr->mgr->get_decompress_sizes_async(j.in_ptrs, j.in_sizes, j.out_sizes, j.statuses, ctl.njobs, stream);
      if (s != Status::SUCCESS) return c_err(s);
    } else {
      ZhDecArgs a{};
      a.in_ptrs = j.in_ptrs;
      a.in_sizes = j.in_sizes;
      a.out_sizes = j.out_sizes;
      a.statuses = (u32 *)j.statuses;
      a.nvcomp_codes = 1;
      if (zh::launch_decompress_sizes(a, ctl.njobs, stream) != hipSuccess) return kFramesDevice;
    }
    if (zh::frames_sizes_launch(d_stream, size, n, ctl.njobs, base, stream) != hipSuccess || !read_ctl(ctl, base, stream)) return kFramesDevice;
    if (ctl.errkey != ~0ull) {  // the lowest failing frame
      *num_frames = (size_t)(ctl.errkey >> 8);
      *error_offset = ctl.job_err_off;
      return (int)(ctl.errkey & 0xFFu);
    }
    if (ctl.limit) return kFramesInvalid;
  }

  // ---- the table
  if (zh::frames_emit_launch(size, n, (size_t)ctl.nframes, d_table, base, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
    return kFramesDevice;
  *table_bytes = table;
  return 0;
}

}  // extern "C"

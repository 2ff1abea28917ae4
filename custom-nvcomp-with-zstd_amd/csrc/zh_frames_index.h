// zh_frames_index.h — host-side entry points of the frame-index kernels (zh_frames.hip): the
// seek table of a buffer of concatenated frames that has none.
#pragma once
#include "zh_common.h"
#include "zh_frames.h"
#include "zh_seek_format.h"

namespace zh {

// Control block of one call, at the start of the (256-aligned) temp buffer.  The host reads it
// back after the scan (ncand), after the walk (the stream's verdict, the frame and job counts) and
// after the size jobs (errkey, limit).
struct FramesCtl {
  u64 ncand;        // candidate frame starts the scan found
  u64 nframes;      // complete frames; on a malformed stream those before the failing one
  u64 err_off;      // a malformed stream: the failing frame's offset
  u32 status;       // the walk's verdict on the stream (ZH_FRAMES_*)
  u32 njobs;        // frames without a Frame_Content_Size: one size job each
  u32 limit;        // an entry field over the seek table format's limit
  u32 pad;
  u64 errkey;       // min over failed size jobs of (entry << 8 | code); ~0: none
  u64 job_err_off;  // the offset of that job's frame
};

// The size jobs (the size pass's device arrays), inside the temp buffer
struct FramesJobs {
  const void **in_ptrs;
  size_t *in_sizes;
  size_t *out_sizes;
  int *statuses;
};

// max_frames: already clamped to ZH_SEEK_MAX_FRAMES.  Candidate capacity: ZH_FRAMES_CANDIDATES.
size_t frames_temp_bytes(size_t stream_bytes, size_t max_frames);
FramesJobs frames_jobs(u8 *base, size_t stream_bytes, size_t max_frames);

// Everything below is enqueued on `stream`, nothing is synchronised.  base: the 256-aligned temp.
// The control block zeroed and the candidates counted: ctl->ncand.
hipError_t frames_count_launch(const void *d_stream, size_t size, size_t max_frames, u8 *base, hipStream_t stream);
// The speculative index (ncand <= the capacity): candidates written in ascending order, one span
// per candidate, pointer doubling from candidate 0, and the reachable frames' entries and jobs.
// split (optional, 5 events): recorded after the write, span, reach and collect kernels, [0] before.
hipError_t frames_reach_launch(const void *d_stream, size_t size, size_t max_frames, size_t ncand, u8 *base, hipEvent_t *split,
                               hipStream_t stream);
// The serial walker: the same entries, jobs and verdict, frame after frame.
hipError_t frames_walk_launch(const void *d_stream, size_t size, size_t max_frames, u8 *base, hipStream_t stream);
// After the size pass: every job's size into its entry, the lowest failing job into the control block.
hipError_t frames_sizes_launch(const void *d_stream, size_t size, size_t max_frames, u32 njobs, u8 *base, hipStream_t stream);
// The table: header, nframes entries, footer (descriptor 0).
hipError_t frames_emit_launch(size_t size, size_t max_frames, size_t nframes, void *d_table, u8 *base, hipStream_t stream);

}  // namespace zh

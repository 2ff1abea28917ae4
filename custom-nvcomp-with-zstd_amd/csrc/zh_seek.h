// zh_seek.h — host-side entry points of the seekable-stream kernels (zh_seek.hip).
#pragma once
#include "zh_common.h"
#include "zh_seek_format.h"
#include "zh_seek_ranges.h"

namespace zh {

// ---- pack ------------------------------------------------------------------------------------
size_t seek_pack_temp_bytes(size_t nframes);
// Everything is enqueued on `stream`; nothing is synchronised.  temp: seek_pack_temp_bytes(n).
hipError_t seek_pack_launch(const void *const *d_frame_ptrs, const size_t *d_frame_sizes, const int *d_frame_statuses,
                            const void *const *d_uncompressed_ptrs, const size_t *d_uncompressed_sizes, size_t nframes,
                            size_t max_compressed_chunk_bytes, int with_checksums, void *d_out, size_t out_capacity, size_t *d_out_size,
                            int *d_status, void *d_temp, hipStream_t stream);

// ---- read ------------------------------------------------------------------------------------
// Control block of one read, at the start of the (256-aligned) temp buffer: the host reads it
// back after the index kernels (job count, status) and after the trim kernel (errkey).
struct SeekReadCtl {
  u32 status;   // nvcomp-style code of the table / range validation
  u32 njobs;    // frames to decode
  u64 total_c;  // sum of Compressed_Size
  u64 total_u;  // sum of Decompressed_Size
  u32 max_d;    // largest Decompressed_Size
  u32 bad;      // a field over the format's limit, or a wrong skippable header
  u64 errkey;   // min over failed jobs of (frame index << 8 | code); ~0: none
};

// Job arrays of a read (the decoder's device arrays), inside the temp buffer's fixed part.
struct SeekJobs {
  const void **in_ptrs;
  size_t *in_sizes;
  void **out_ptrs;
  size_t *out_caps;
  size_t *out_sizes;
  int *statuses;
  void *meta;
};

// Temp buffer of a read: a fixed part sized by the table's N (control block, the two scanned
// size columns, the job arrays), then two bounce slots of align256(max_d) bytes, then the
// decoder's workspace for njobs items.
size_t seek_read_fixed_bytes(size_t nframes);
size_t seek_read_bounce_bytes(size_t max_frame_uncompressed);
SeekJobs seek_read_jobs(u8 *base, size_t nframes);

// Parse + validate the table on the device, scan both columns and emit the decode jobs of
// [offset, offset + length).  base: the 256-aligned temp buffer.
// entry: bytes per table entry, from the footer's descriptor as the host read it.
hipError_t seek_index_launch(const void *d_stream, size_t size, size_t nframes, u32 entry, u64 offset, u64 length, void *d_out, u8 *base,
                             hipStream_t stream);
// Check every job's decode, verify checksums when asked and the table has them, and copy the
// bounced edge frames' overlap into d_out.
hipError_t seek_trim_launch(const void *d_stream, size_t size, size_t nframes, u32 entry, u32 njobs, u64 offset, u64 length, void *d_out,
                            int verify, u8 *base, hipStream_t stream);

// ---- read of many ranges ---------------------------------------------------------------------
// Temp buffer of a batched read (zh_seek_ranges.h): the fixed part of a read, the arrays sized by
// N and by the number of ranges, `jobs` staging slots of align256(max_d) bytes, dec_bytes of
// decoder workspace.  Everything in front of the staging slots depends on N and the ranges only.
ZhSeekRangesLayout seek_ranges_layout(size_t nframes, size_t num_ranges, size_t jobs, size_t max_d, size_t dec_bytes);
// Parse + validate + scan the table as a read does, then give every range its verdict and its
// first and last entry, mark the entries the ranges touch and emit one decode job (into a
// staging slot) per marked entry with content.  The control block holds the table's status and
// the job count.  No range status and no destination is written.
hipError_t seek_ranges_index_launch(const void *d_stream, size_t size, size_t nframes, u32 entry, const unsigned long long *d_offsets,
                                    const size_t *d_lengths, size_t num_ranges, size_t max_length, u8 *base, hipStream_t stream);
// After the decoder: check every job, write every range's status, and copy the bytes of the
// ranges that touch only good frames to their destinations.
hipError_t seek_ranges_finish_launch(const void *d_stream, size_t size, size_t nframes, u32 entry, u32 njobs,
                                     const unsigned long long *d_offsets, const size_t *d_lengths, void *const *d_out_ptrs, size_t num_ranges,
                                     size_t max_length, int verify, int *d_range_statuses, u8 *base, hipStream_t stream);

// ---- info ------------------------------------------------------------------------------------
struct SeekInfoRes {
  u64 total_c, total_u;
  u32 max_d, bad;
};
// d_res must be zeroed (stream-ordered) before the launch.
hipError_t seek_info_launch(const void *d_stream, size_t size, size_t nframes, SeekInfoRes *d_res, hipStream_t stream);

}  // namespace zh

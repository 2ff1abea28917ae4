// zh_host_seek.cpp — host runtime, the seekable-stream drivers (C entries).
#include "zh_host.h"
#include "zh_seek.h"

using namespace cuda_zstd;

// The codes c_err gives these statuses; the returns that use them leave the last-error slot alone
using nvcomp_v5::status_to_nvcomp_error;
static int const kSeekInvalid = status_to_nvcomp_error(Status::ERROR_INVALID_PARAMETER), kSeekOom = status_to_nvcomp_error(Status::ERROR_OUT_OF_MEMORY),
                 kSeekDevice = status_to_nvcomp_error(Status::ERROR_CUDA_ERROR), kSeekCorrupt = status_to_nvcomp_error(Status::ERROR_CORRUPT_DATA),
                 kSeekTooSmall = status_to_nvcomp_error(Status::ERROR_BUFFER_TOO_SMALL);

extern "C" {
// ---- seekable streams (zh_seek.hip; format in zh_seek_format.h) -------------------------------
size_t cuda_zstd_seekable_max_size(size_t num_frames, size_t max_compressed_chunk_bytes, int with_checksums) {
  return num_frames * max_compressed_chunk_bytes + (size_t)zh_seek_table_bytes(num_frames, with_checksums);
}
size_t cuda_zstd_seekable_pack_get_temp_size(size_t num_frames) { return zh::seek_pack_temp_bytes(num_frames); }

int cuda_zstd_seekable_pack_async(const void *const *d_frame_ptrs, const size_t *d_frame_sizes, const int *d_frame_statuses,
                                  const void *const *d_uncompressed_ptrs, const size_t *d_uncompressed_sizes, size_t num_frames,
                                  size_t max_compressed_chunk_bytes, int with_checksums, void *d_out, size_t out_capacity, size_t *d_out_size,
                                  int *d_status, void *d_temp, size_t temp_bytes, hipStream_t stream) {
  if (!d_out || !d_out_size || !d_status || num_frames > ZH_SEEK_MAX_FRAMES) return c_err(Status::ERROR_INVALID_PARAMETER);
  if (num_frames && (!d_frame_ptrs || !d_frame_sizes || !d_uncompressed_sizes || max_compressed_chunk_bytes == 0 ||
                     (with_checksums && !d_uncompressed_ptrs)))
    return c_err(Status::ERROR_INVALID_PARAMETER);
  if (!d_temp || temp_bytes < zh::seek_pack_temp_bytes(num_frames)) return c_err(Status::ERROR_BUFFER_TOO_SMALL);
  hipError_t const e = zh::seek_pack_launch(d_frame_ptrs, d_frame_sizes, d_frame_statuses, d_uncompressed_ptrs, d_uncompressed_sizes, num_frames,
                                            max_compressed_chunk_bytes, with_checksums != 0, d_out, out_capacity, d_out_size, d_status, d_temp,
                                            stream);
  return e == hipSuccess ? 0 : c_err(Status::ERROR_CUDA_ERROR);
}

// The last 9 bytes of a stream in host or device memory, parsed on the host (the one small word
// the read and info calls fetch; the table itself stays where it is).
static int seek_fetch_footer(const void *buf, size_t size, bool dev, ZhSeekFooter &f, hipStream_t stream) {
  if (!buf) return kSeekInvalid;
  if (size < ZH_SEEK_OVERHEAD) return kSeekCorrupt;
  u8 foot[ZH_SEEK_FOOTER];
  if (dev) {
    if (hipMemcpyAsync(foot, (const u8 *)buf + size - ZH_SEEK_FOOTER, ZH_SEEK_FOOTER, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
      return kSeekDevice;
  } else {
    memcpy(foot, (const u8 *)buf + size - ZH_SEEK_FOOTER, ZH_SEEK_FOOTER);
  }
  return (int)zh_seek_parse_footer(foot, size, &f);
}

int cuda_zstd_seekable_info(const void *stream_buf, size_t size, size_t *num_frames, unsigned long long *total_uncompressed,
                            unsigned int *max_frame_uncompressed, int *has_checksums) {
  bool const dev = stream_buf && is_device_ptr(stream_buf);
  ZhSeekFooter f;
  int rc = seek_fetch_footer(stream_buf, size, dev, f, 0);
  if (rc) return rc;
  zh::SeekInfoRes r{};
  if (dev) {
    zh::SeekInfoRes *d_res = nullptr;
    if (hipMalloc((void **)&d_res, sizeof(r)) != hipSuccess) return kSeekOom;
    bool ok = hipMemsetAsync(d_res, 0, sizeof(r), 0) == hipSuccess && zh::seek_info_launch(stream_buf, size, (size_t)f.n, d_res, 0) == hipSuccess &&
              hipMemcpy(&r, d_res, sizeof(r), hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(d_res);
    if (!ok) return kSeekDevice;
  } else {
    const u8 *const table = (const u8 *)stream_buf + (size - f.table);
    if (zh_seek_check_header(table, &f) != ZH_SEEK_OK) r.bad = 1;
    for (u64 i = 0; i < f.n; i++) {
      u64 const c = zh_seek_ld32(table + 8 + i * f.entry), d = zh_seek_ld32(table + 8 + i * f.entry + 4);
      if (!zh_seek_field_ok(c) || !zh_seek_field_ok(d)) { r.bad = 1; break; }
      r.total_c += c;
      r.total_u += d;
      r.max_d = std::max(r.max_d, (u32)d);
    }
  }
  if (r.bad || r.total_c + f.table != size) return kSeekCorrupt;
  if (num_frames) *num_frames = (size_t)f.n;
  if (total_uncompressed) *total_uncompressed = r.total_u;
  if (max_frame_uncompressed) *max_frame_uncompressed = r.max_d;
  if (has_checksums) *has_checksums = (int)f.checksums;
  return 0;
}

// Temp of a read that decodes at most max_jobs frames (max_jobs = num_frames always suffices)
size_t cuda_zstd_seekable_read_get_temp_size_jobs(size_t num_frames, size_t max_jobs, size_t max_frame_uncompressed) {
  return zh::seek_read_fixed_bytes(num_frames) + zh::seek_read_bounce_bytes(max_frame_uncompressed) +
         ZstdBatchManager::get_batch_device_decompress_temp_size(std::min(max_jobs, num_frames), std::max<size_t>(max_frame_uncompressed, 1)) + 256;
}
size_t cuda_zstd_seekable_read_get_temp_size(size_t num_frames, size_t max_frame_uncompressed) {
  return cuda_zstd_seekable_read_get_temp_size_jobs(num_frames, num_frames, max_frame_uncompressed);
}

int cuda_zstd_seekable_read(nvcomp_zstd_batch_manager_t *mgr, const void *d_stream, size_t size, unsigned long long offset, size_t length,
                            void *d_out, size_t *written, int verify_checksums, void *d_temp, size_t temp_bytes, hipStream_t stream) {
  if (written) *written = 0;
  if (!mgr || !mgr->mgr || !d_stream || (length && !d_out)) return c_err(Status::ERROR_INVALID_PARAMETER);
  ZhSeekFooter f;
  int rc = seek_fetch_footer(d_stream, size, true, f, stream);
  if (rc) return rc;
  size_t const n = (size_t)f.n, fixed = zh::seek_read_fixed_bytes(n);
  if (!d_temp || temp_bytes < fixed + 256) return kSeekTooSmall;  // nothing launched
  u8 *const base = aligned_base(d_temp);
  size_t const avail = temp_bytes - (size_t)(base - (u8 *)d_temp);
  if (zh::seek_index_launch(d_stream, size, n, f.entry, offset, length, d_out, base, stream) != hipSuccess) return kSeekDevice;
  zh::SeekReadCtl ctl;
  if (hipMemcpyAsync(&ctl, base, sizeof(ctl), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return kSeekDevice;
  if (ctl.status) return (int)ctl.status;
  if (ctl.njobs == 0) return 0;  // length 0 (a valid table, nothing to decode)
  // the decoder's workspace follows the bounce slots; sized now that the job count is known
  size_t const bounce = zh::seek_read_bounce_bytes(ctl.max_d), max_out = std::max<size_t>(ctl.max_d, 1);
  size_t const dec = ZstdBatchManager::get_batch_device_decompress_temp_size(ctl.njobs, max_out);
  if (ctl.njobs > n || avail < fixed + bounce + dec) return kSeekTooSmall;  // the decoder is not launched
  zh::SeekJobs const j = zh::seek_read_jobs(base, n);
  Status const s = mgr->mgr->batch_manager().decompress_batch_device(j.in_ptrs, j.in_sizes, j.out_caps, max_out, ctl.njobs, j.out_ptrs, j.out_sizes,
                                                                     j.statuses, base + fixed + bounce, dec, stream);
  if (s != Status::SUCCESS) return c_err(s);
  if (zh::seek_trim_launch(d_stream, size, n, f.entry, ctl.njobs, offset, length, d_out, verify_checksums, base, stream) != hipSuccess) return kSeekDevice;
  if (hipMemcpyAsync(&ctl, base, sizeof(ctl), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return kSeekDevice;
  if (ctl.errkey != ~0ull) return (int)(ctl.errkey & 0xFFu);
  if (written) *written = length;
  return 0;
}

// Temp of a batched read whose ranges touch at most max_jobs frames with content
size_t cuda_zstd_seekable_read_ranges_get_temp_size(size_t num_frames, size_t num_ranges, size_t max_jobs, size_t max_frame_uncompressed) {
  size_t const jobs = std::min(max_jobs, num_frames);
  size_t const dec = ZstdBatchManager::get_batch_device_decompress_temp_size(jobs, std::max<size_t>(max_frame_uncompressed, 1));
  return zh::seek_ranges_layout(num_frames, num_ranges, jobs, max_frame_uncompressed, dec).total;
}

int cuda_zstd_seekable_read_ranges(nvcomp_zstd_batch_manager_t *mgr, const void *d_stream, size_t size, const unsigned long long *d_offsets,
                                   const size_t *d_lengths, void *const *d_out_ptrs, size_t num_ranges, size_t max_length, int verify_checksums,
                                   int *d_range_statuses, size_t *frames_decoded, void *d_temp, size_t temp_bytes, hipStream_t stream) {
  if (frames_decoded) *frames_decoded = 0;
  if (!mgr || !mgr->mgr || !d_stream) return c_err(Status::ERROR_INVALID_PARAMETER);
  if (num_ranges == 0) return 0;
  if (!d_offsets || !d_lengths || !d_out_ptrs || !d_range_statuses) return c_err(Status::ERROR_INVALID_PARAMETER);
  ZhSeekFooter f;
  int rc = seek_fetch_footer(d_stream, size, true, f, stream);
  if (rc) return rc;
  size_t const n = (size_t)f.n;
  // the part in front of the staging slots depends on the table and the ranges alone
  if (!d_temp || temp_bytes < zh::seek_ranges_layout(n, num_ranges, 0, 0, 0).staging + 256) return kSeekTooSmall;  // nothing launched
  u8 *const base = aligned_base(d_temp);
  if (zh::seek_ranges_index_launch(d_stream, size, n, f.entry, d_offsets, d_lengths, num_ranges, max_length, base, stream) != hipSuccess) return kSeekDevice;
  zh::SeekReadCtl ctl;
  if (hipMemcpyAsync(&ctl, base, sizeof(ctl), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return kSeekDevice;
  if (ctl.status) return (int)ctl.status;
  // the staging slots and the decoder's workspace, sized now that the job count is known: the
  // buffer must be what get_temp_size asks for this many jobs
  size_t const max_out = std::max<size_t>(ctl.max_d, 1);
  size_t const dec = ctl.njobs ? ZstdBatchManager::get_batch_device_decompress_temp_size(ctl.njobs, max_out) : 0;
  ZhSeekRangesLayout const L = zh::seek_ranges_layout(n, num_ranges, ctl.njobs, ctl.max_d, dec);
  if (ctl.njobs > n || (ctl.njobs && temp_bytes < L.total)) return kSeekTooSmall;  // the decoder is not launched
  if (ctl.njobs) {
    zh::SeekJobs const j = zh::seek_read_jobs(base, n);
    Status const s = mgr->mgr->batch_manager().decompress_batch_device(j.in_ptrs, j.in_sizes, j.out_caps, max_out, ctl.njobs, j.out_ptrs, j.out_sizes,
                                                                       j.statuses, base + L.dec, dec, stream);
    if (s != Status::SUCCESS) return c_err(s);
  }
  // (no range longer than the content is copied: the scatter grid is sized by the smaller bound)
  if (zh::seek_ranges_finish_launch(d_stream, size, n, f.entry, ctl.njobs, d_offsets, d_lengths, d_out_ptrs, num_ranges,
                                    (size_t)std::min<u64>(max_length, ctl.total_u), verify_checksums, d_range_statuses, base, stream) != hipSuccess)
    return kSeekDevice;
  if (hipStreamSynchronize(stream) != hipSuccess) return kSeekDevice;
  if (frames_decoded) *frames_decoded = ctl.njobs;
  return 0;
}

}  // extern "C"

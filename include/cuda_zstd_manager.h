// cuda_zstd_manager.h — manager interface of the gfx950 Zstandard compressor.
//
// Same class names, virtual signatures and semantics as the reference's
// include/cuda_zstd_manager.h:
//   ZstdManager          :45-100   (pure-virtual interface)
//   ZstdBatchManager     :113-278  (compress_batch, inference decompress API)
//   ZstdStreamingManager :300-352  (each chunk an independent frame, as in the reference)
//   factories            :358-363, convenience :369-386, utilities :392-419
// The C ABI of the same header (:433-479) lives in cuda_zstd_capi.h.
#ifndef CUDA_ZSTD_MANAGER_H_
#define CUDA_ZSTD_MANAGER_H_

#include "cuda_zstd_types.h"
#include "cuda_zstd_capi.h"
#include "cuda_zstd_dictionary.h"

#ifdef __cplusplus
#include <memory>
#include <vector>

namespace cuda_zstd {

class ZstdManager {
 public:
  virtual ~ZstdManager() = default;
  virtual Status configure(const CompressionConfig &config) = 0;
  virtual CompressionConfig get_config() const = 0;
  virtual size_t get_compress_temp_size(size_t uncompressed_size) const = 0;
  virtual size_t get_decompress_temp_size(size_t compressed_size) const = 0;
  virtual size_t get_max_compressed_size(size_t uncompressed_size) const = 0;
  virtual Status compress(const void *uncompressed_data, size_t uncompressed_size, void *compressed_data, size_t *compressed_size,
                          void *temp_workspace, size_t temp_size, const void *dict_buffer, size_t dict_size, hipStream_t stream,
                          void *streaming_context = nullptr) = 0;
  virtual Status decompress(const void *compressed_data, size_t compressed_size, void *uncompressed_data, size_t *uncompressed_size,
                            void *temp_workspace, size_t temp_size, hipStream_t stream = 0) = 0;
  virtual Status set_dictionary(const dictionary::Dictionary &dict) = 0;
  virtual Status get_dictionary(dictionary::Dictionary &dict) const = 0;
  virtual Status clear_dictionary() = 0;
  virtual const CompressionStats &get_stats() const = 0;
  virtual Status set_compression_level(int level) = 0;
  virtual int get_compression_level() const = 0;
  virtual void reset_stats() = 0;

  enum class ExecutionPath { CPU, GPU_BATCH, GPU_CHUNK };
  // reference src/cuda_zstd_manager.cu:6465-6471: size < threshold -> CPU
  static ExecutionPath select_execution_path(size_t size, int cpu_threshold = 0);
  virtual Status preallocate_tables(hipStream_t stream = 0) { (void)stream; return Status::SUCCESS; }
  virtual Status free_tables(hipStream_t stream = 0) { (void)stream; return Status::SUCCESS; }
};

// A set of dictionaries on the device, for batches whose chunks use different dictionaries (one per
// table, tenant, column or schema version): ZstdBatchManager::set_dictionary_set binds it, and
// compress_batch_device_dicts takes one entry index per chunk.  Created from 1 .. 4,096
// dictionaries (raw content or formatted, MIN_DICT_SIZE .. MAX_DICT_SIZE bytes each, host or device
// memory; the bytes are copied, so the sources may go away), each with everything set_dictionary
// builds for one dictionary -- the matchers' tables of its content and, for a formatted dictionary,
// the encoder's view of its entropy section -- in one device allocation of about 0.5 MiB per 64 KiB
// dictionary.  Immutable.  Two entries with the same non-zero Dictionary_ID are refused
// (ERROR_INVALID_PARAMETER); raw-content entries (ID 0) are reachable by index only.  Destruction
// waits for the stream-ordered calls that read the set.
class DictionarySet {
 public:
  static Status create(const dictionary::Dictionary *const *dicts, size_t count, hipStream_t stream, std::unique_ptr<DictionarySet> &out);
  ~DictionarySet();
  size_t count() const;
  // entry index of a non-zero Dictionary_ID, or -1
  int find(u32 dictionary_id) const;
  class Impl;
  const Impl &impl() const { return *pimpl_; }

 private:
  DictionarySet();
  std::unique_ptr<Impl> pimpl_;
};

class ZstdBatchManager : public ZstdManager {
 public:
  ZstdBatchManager();
  explicit ZstdBatchManager(const CompressionConfig &config);
  ~ZstdBatchManager() override;

  Status configure(const CompressionConfig &config) override;
  CompressionConfig get_config() const override;
  size_t get_compress_temp_size(size_t uncompressed_size) const override;
  size_t get_decompress_temp_size(size_t compressed_size) const override;
  size_t get_max_compressed_size(size_t uncompressed_size) const override;
  Status compress(const void *uncompressed_data, size_t uncompressed_size, void *compressed_data, size_t *compressed_size,
                  void *temp_workspace, size_t temp_size, const void *dict_buffer, size_t dict_size, hipStream_t stream = 0,
                  void *streaming_context = nullptr) override;
  Status decompress(const void *compressed_data, size_t compressed_size, void *uncompressed_data, size_t *uncompressed_size,
                    void *temp_workspace, size_t temp_size, hipStream_t stream = 0) override;
  Status set_dictionary(const dictionary::Dictionary &dict) override;
  Status get_dictionary(dictionary::Dictionary &dict) const override;
  Status clear_dictionary() override;
  const CompressionStats &get_stats() const override;
  Status set_compression_level(int level) override;
  int get_compression_level() const override;
  void reset_stats() override;

  Status compress_batch(const std::vector<BatchItem> &items, void *temp_workspace, size_t temp_size, hipStream_t stream = 0);
  Status decompress_batch(const std::vector<BatchItem> &items, void *temp_workspace, size_t temp_size, hipStream_t stream = 0);
  size_t get_batch_compress_temp_size(const std::vector<size_t> &uncompressed_sizes) const;
  size_t get_batch_decompress_temp_size(const std::vector<size_t> &compressed_sizes) const;

  Status decompress_to_preallocated(const void *compressed_data, size_t compressed_size, void *preallocated_output,
                                    size_t output_capacity, size_t *actual_output_size, void *temp_workspace, size_t temp_size,
                                    hipStream_t stream = 0);
  Status decompress_batch_preallocated(std::vector<BatchItem> &items, void *temp_workspace, size_t temp_size, hipStream_t stream = 0);
  Status decompress_async_no_sync(const void *compressed_data, size_t compressed_size, void *preallocated_output,
                                  size_t output_capacity, size_t *d_actual_size, void *temp_workspace, size_t temp_size,
                                  hipStream_t stream);
  size_t get_inference_workspace_size(size_t max_compressed_size, size_t max_output_size) const;
  Status allocate_inference_workspace(size_t max_compressed_size, size_t max_output_size, void **workspace_ptr, size_t *workspace_size);
  Status free_inference_workspace(void *workspace_ptr);

  // Stream-ordered batched compression over device arrays (no host sync); used by the
  // nvcomp_zstd_batched_compress_async_v5 C entry.
  Status compress_batch_device(const void *const *d_in_ptrs, const size_t *d_in_sizes, size_t max_chunk_bytes, size_t count,
                               void *const *d_out_ptrs, size_t *d_out_sizes, int *d_statuses, void *temp_workspace, size_t temp_size,
                               hipStream_t stream);
  // levels below 5 (ZH_DEEP_LEVEL) without a dictionary; otherwise get_batch_device_temp_size_for
  static size_t get_batch_device_temp_size(size_t count, size_t max_chunk_bytes);
  // the same for this manager's level and dictionary (levels >= 5 add the deep matcher's scratch
  // slots, ~1.2 MB per persistent workgroup; a dictionary over 32 KiB chunks adds history blocks)
  size_t get_batch_device_temp_size_for(size_t count, size_t max_chunk_bytes) const;
  // The same call with one level per chunk, read on the device: d_levels[i] (a device int array,
  // such as the one cuda_zstd_adaptive_analyze_batch_async leaves behind) is chunk i's level, and
  // frame i is byte-identical to what a manager at that level writes for chunk i through
  // compress_batch_device with the same max_chunk_bytes.  Stream-ordered like it: no allocation, no
  // synchronisation, no copy to the host.  The manager's level is not used; its checksum setting
  // applies.  A level outside 1..22 gives that chunk size 0 and status ERROR_INVALID_PARAMETER and
  // leaves its output untouched; the other chunks are unaffected.  ERROR_INVALID_PARAMETER for a null
  // array, max_chunk_bytes == 0, a manager with a dictionary set or count > 1,048,576;
  // ERROR_BUFFER_TOO_SMALL for a
  // workspace below get_batch_device_levels_temp_size (nothing is launched); count == 0 succeeds.
  // Not covered: dictionaries (a dictionary frame's block split depends on its level), dict_entropy,
  // long-distance matching, the streaming manager.
  Status compress_batch_device_levels(const void *const *d_in_ptrs, const size_t *d_in_sizes, const int *d_levels, size_t max_chunk_bytes,
                                      size_t count, void *const *d_out_ptrs, size_t *d_out_sizes, int *d_statuses, void *temp_workspace,
                                      size_t temp_size, hipStream_t stream);
  // its workspace: get_batch_device_temp_size_for of a level >= 5 plus the items' ranks, one level
  // byte per block and the class ranges; at least what any dictionary-less manager's call needs
  static size_t get_batch_device_levels_temp_size(size_t count, size_t max_chunk_bytes);
  // compress_batch_device with one prefix per chunk: d_prefix_ptrs[i] / d_prefix_sizes[i] (device
  // arrays) are the bytes that precede chunk i, used as a raw-content dictionary without a
  // Dictionary_ID.  Frame i is byte-identical to what compress_with_history(chunk i, prefix i) writes
  // at this manager's configuration; with d_prefix_sizes[i] == 0 it is compress_batch_device's frame.
  // Stream-ordered like it: no allocation, no synchronisation, no copy to the host.  Only the tail
  // the matcher stages is read: below level 5 the last 64 KiB - block bytes (a chunk over 32 KiB is
  // cut into 32 KiB blocks, the first behind the prefix's last 32 KiB, later ones behind the frame's
  // previous 32 KiB), from level 5 on the last 64 KiB.  A non-zero prefix size with a null pointer
  // gives that chunk size 0 and status ERROR_INVALID_PARAMETER and leaves its output untouched.
  // ERROR_INVALID_PARAMETER for a null array, max_chunk_bytes == 0 or a manager with a dictionary
  // set; ERROR_BUFFER_TOO_SMALL for a workspace below get_batch_device_prefix_temp_size (nothing is
  // launched); count == 0 succeeds.  The checksum setting applies; dict_entropy and enable_ldm have
  // no effect here.
  // Not covered: a prefix together with a manager dictionary, with per-chunk levels, or with
  // dict_entropy / long-distance matching; staging the aligned region of a reference for blocks
  // after the first (below level 5 a 64 KiB chunk's second block sees the frame's own first half,
  // not the reference's second half: delta users there should keep chunks <= 32 KiB; lifting that
  // needs an offset bias through the matcher and the sequence stage).
  Status compress_batch_device_prefix(const void *const *d_in_ptrs, const size_t *d_in_sizes, const void *const *d_prefix_ptrs,
                                      const size_t *d_prefix_sizes, size_t max_chunk_bytes, size_t count, void *const *d_out_ptrs,
                                      size_t *d_out_sizes, int *d_statuses, void *temp_workspace, size_t temp_size, hipStream_t stream);
  // its workspace: that of a manager with a dictionary at this level (the 32 KiB split with staging
  // and gather above 32 KiB below level 5, the deep matcher's slots from level 5 on)
  size_t get_batch_device_prefix_temp_size(size_t count, size_t max_chunk_bytes) const;
  // A batch against a set of dictionaries.  set_dictionary_set binds a set (null: none) for the
  // calls below and for the decoding entries; the manager keeps the set's device memory alive while
  // bound.  Not together with set_dictionary: either one while the other is in place is
  // ERROR_INVALID_PARAMETER.
  Status set_dictionary_set(const DictionarySet *set);
  // compress_batch_device with one entry of the bound set per chunk: d_dict_index[i] (a device int32
  // array, read on the device) names chunk i's dictionary, -1 none.  Frame i is byte-identical to
  // what a manager at this level, checksum and dict_entropy setting with that one dictionary set
  // writes for chunk i through compress_batch_device (it carries the entry's Dictionary_ID, starts
  // from the entry's precomputed tables and, with dict_entropy, may use its entropy section); -1
  // gives the frame of a manager without a dictionary.  An index below -1 or past the set gives that
  // chunk size 0 and status ERROR_INVALID_PARAMETER and leaves its output untouched.  Stream-ordered:
  // no allocation, no synchronisation, no copy to the host, and the same launches whatever the set's
  // size or the mix.  ERROR_INVALID_PARAMETER without a bound set, for a null array, max_chunk_bytes
  // == 0 or enable_ldm; ERROR_BUFFER_TOO_SMALL for a workspace below get_batch_device_dicts_temp_size
  // (nothing is launched); count == 0 succeeds.
  // Not covered: a set together with per-chunk levels, with a per-chunk prefix, with long-distance
  // matching, and the streaming managers.
  Status compress_batch_device_dicts(const void *const *d_in_ptrs, const size_t *d_in_sizes, const int32_t *d_dict_index, size_t max_chunk_bytes,
                                     size_t count, void *const *d_out_ptrs, size_t *d_out_sizes, int *d_statuses, void *temp_workspace,
                                     size_t temp_size, hipStream_t stream);
  // its workspace: get_batch_device_prefix_temp_size's (the index array is read where it is)
  size_t get_batch_device_dicts_temp_size(size_t count, size_t max_chunk_bytes) const;

  // Stream-ordered batched decompression over device arrays (no host sync; GPU decoder,
  // any RFC 8878 frames); used by nvcomp_zstd_batched_decompress_async_v5.
  // d_out_caps[i] = output capacity (every capacity <= max_uncompressed_chunk_bytes, or null:
  // max_uncompressed_chunk_bytes for all); d_out_sizes[i] = bytes produced (0 on error);
  // d_statuses[i] (optional) = nvcomp-style code.
  Status decompress_batch_device(const void *const *d_in_ptrs, const size_t *d_in_sizes, const size_t *d_out_caps,
                                 size_t max_uncompressed_chunk_bytes, size_t count, void *const *d_out_ptrs, size_t *d_out_sizes,
                                 int *d_statuses, void *temp_workspace, size_t temp_size, hipStream_t stream);
  static size_t get_batch_device_decompress_temp_size(size_t count, size_t max_uncompressed_chunk_bytes);
  // decompress_batch_device with one prefix per buffer (device arrays; size 0 or a null pointer:
  // none): the whole prefix is addressable in front of the frame, as with libzstd's
  // ZSTD_decompress_usingDict on raw content.  A frame that names a Dictionary_ID is answered with
  // the dictionary-wrong code (there is no formatted dictionary on this route).  Same workspace;
  // ERROR_INVALID_PARAMETER for a manager with a dictionary set.
  Status decompress_batch_device_prefix(const void *const *d_in_ptrs, const size_t *d_in_sizes, const void *const *d_prefix_ptrs,
                                        const size_t *d_prefix_sizes, const size_t *d_out_caps, size_t max_uncompressed_chunk_bytes,
                                        size_t count, void *const *d_out_ptrs, size_t *d_out_sizes, int *d_statuses, void *temp_workspace,
                                        size_t temp_size, hipStream_t stream);
  // Decoding against the bound dictionary set.  With a set bound, decompress_batch_device and
  // get_decompressed_sizes_async resolve every frame's dictionary on the device from its
  // Dictionary_ID (per frame: a buffer may hold frames naming different dictionaries); this entry
  // adds d_dict_index, a device int32 array or null: -1 (or null) resolves by ID, an index >= 0 uses
  // that entry -- the way to name a raw-content entry, whose frames carry no ID -- and an index
  // outside the set makes the buffer ERROR_INVALID_PARAMETER.  A non-zero ID that is not in the set,
  // or that differs from the named entry's, is answered with the dictionary-wrong code; a frame
  // without an ID and without an index is decoded without a dictionary; with an index the entry's
  // content precedes it, and a formatted entry's tables and repcodes seed it.  Same workspace as
  // decompress_batch_device; ERROR_INVALID_PARAMETER without a bound set.
  Status decompress_batch_device_dicts(const void *const *d_in_ptrs, const size_t *d_in_sizes, const int32_t *d_dict_index,
                                       const size_t *d_out_caps, size_t max_uncompressed_chunk_bytes, size_t count, void *const *d_out_ptrs,
                                       size_t *d_out_sizes, int *d_statuses, void *temp_workspace, size_t temp_size, hipStream_t stream);
  // The decompressed size of every buffer, computed on the device (nvCOMP's
  // nvcompBatchedZstdGetDecompressSizeAsync): all arrays are device arrays, one launch, no
  // workspace, no allocation, no synchronisation.  d_out_sizes[i] = the bytes all frames of buffer i
  // regenerate: a frame's Frame_Content_Size where it has one (believed, as libzstd's
  // ZSTD_findDecompressedSize does), else summed from its blocks, so frames of streaming writers
  // are answered exactly too.  d_statuses[i] (optional) = Status value, or nvcomp code when
  // nvcomp_codes; the size is 0 where the status is not success.  For every buffer the decoder
  // accepts this is exactly what it produces; an empty or null buffer is ERROR_INVALID_PARAMETER.
  // The manager's dictionary is used as in decompress_batch_device.
  Status get_decompressed_sizes_async(const void *const *d_ptrs, const size_t *d_sizes, size_t count, size_t *d_out_sizes, int *d_statuses,
                                      hipStream_t stream, bool nvcomp_codes = false);

  // Streaming history (what the reference's compress_chunk_with_history does by
  // passing its device window as a raw-content dictionary, src/cuda_zstd_manager.cu:6327-6418):
  // d_history = device-resident preceding bytes (no copy), used as the frame's history; frames
  // decode with that history as a raw-content dictionary (libzstd ZSTD_decompress_usingDict too).
  Status compress_with_history(const void *uncompressed_data, size_t uncompressed_size, void *compressed_data, size_t *compressed_size,
                               void *temp_workspace, size_t temp_size, const void *d_history, size_t history_size, hipStream_t stream = 0);
  Status decompress_with_history(const void *compressed_data, size_t compressed_size, void *uncompressed_data, size_t *uncompressed_size,
                                 void *temp_workspace, size_t temp_size, const void *d_history, size_t history_size, hipStream_t stream = 0);

  // Long-distance matching (config.enable_ldm): what compress() of this device buffer
  // would split, one record per 32 KiB cell = {first byte of the run, its length (0: the cell is
  // not split), distance}, three u32 each, copied to host_records (capacity in records).
  // *num_records = cells.  temp_workspace as for compress() of the same size with enable_ldm set.
  // Frames the long-distance plan does not apply to (one block, or over 4 GiB) report 0 records.
  // Statistics pass of dictionary finalisation (dictionary::finalize_dictionary): the device
  // buffers in d_ptrs (a host array of `count` device pointers; sizes[i] > 0 bytes each) are
  // compressed as records against the manager's dictionary at its level, and the entropy kernel
  // adds every block's literal histogram and LL / OF / ML code counts into counts[448] (host):
  // literal bytes [0, 256), LL [256, 320), OF [320, 384), ML [384, 448).  The frames are dropped.
  // Integer atomics: the counts do not depend on scheduling.  Blocks until done; temp memory is
  // the function's own.
  Status collect_entropy_stats(const void *const *d_ptrs, const size_t *sizes, size_t count, unsigned int *counts, hipStream_t stream = 0);
  Status ldm_plan(const void *d_src, size_t size, unsigned int *host_records, size_t capacity, size_t *num_records, void *temp_workspace,
                  size_t temp_size, hipStream_t stream = 0);

 private:
  class Impl;
  std::unique_ptr<Impl> pimpl_;
};

class ZstdStreamingManager {
 public:
  ZstdStreamingManager();
  explicit ZstdStreamingManager(const CompressionConfig &config);
  ~ZstdStreamingManager();
  Status init_compression(hipStream_t stream = 0, size_t max_chunk_size = 0);
  Status init_compression_with_history(hipStream_t stream = 0, size_t max_chunk_size = 0);
  Status init_decompression(hipStream_t stream = 0);
  // (not in the reference) a decode-only session whose frames came from
  // compress_chunk_with_history: with a raw-content dictionary set, decompress_chunk cannot tell
  // a history frame from a dictionary frame by its header (both carry Dictionary_ID 0)
  Status init_decompression_with_history(hipStream_t stream = 0);
  Status compress_chunk(const void *input, size_t input_size, void *output, size_t *output_size, bool is_last_chunk, hipStream_t stream = 0);
  Status compress_chunk_with_history(const void *input, size_t input_size, void *output, size_t *output_size, bool is_last_chunk,
                                     hipStream_t stream = 0);
  Status decompress_chunk(const void *input, size_t input_size, void *output, size_t *output_size, bool *is_last_chunk,
                          hipStream_t stream = 0);
  Status reset();
  Status reset_streaming();
  Status flush(hipStream_t stream = 0);
  Status flush_streaming(hipStream_t stream = 0);
  Status set_config(const CompressionConfig &config);
  Status set_dictionary(const dictionary::Dictionary &dict);
  CompressionConfig get_config() const;
  size_t get_temp_size() const;
  bool is_compression_initialized() const;
  bool is_decompression_initialized() const;

 private:
  class Impl;
  std::unique_ptr<Impl> pimpl_;
};

std::unique_ptr<ZstdManager> create_manager(int compression_level = 3);
std::unique_ptr<ZstdManager> create_manager(const CompressionConfig &config);
std::unique_ptr<ZstdBatchManager> create_batch_manager(int compression_level = 3);
std::unique_ptr<ZstdStreamingManager> create_streaming_manager(int compression_level = 3);

Status compress_simple(const void *uncompressed_data, size_t uncompressed_size, void *compressed_data, size_t *compressed_size,
                       int compression_level = 3, hipStream_t stream = 0);
Status decompress_simple(const void *compressed_data, size_t compressed_size, void *uncompressed_data, size_t *uncompressed_size,
                         hipStream_t stream = 0);
// reference include/cuda_zstd_manager.h:377-386 (declared there, never defined): one frame
// compressed against / decompressed with `dict` (raw content or RFC 8878 §5 formatted), the
// workspace allocated and freed inside the call, output valid on return
Status compress_with_dict(const void *uncompressed_data, size_t uncompressed_size, void *compressed_data, size_t *compressed_size,
                          const dictionary::Dictionary &dict, int compression_level = 3, hipStream_t stream = 0);
Status decompress_with_dict(const void *compressed_data, size_t compressed_size, void *uncompressed_data, size_t *uncompressed_size,
                            const dictionary::Dictionary &dict, hipStream_t stream = 0);

Status get_decompressed_size(const void *compressed_data, size_t compressed_size, size_t *decompressed_size);
Status validate_compressed_data(const void *compressed_data, size_t compressed_size, bool check_checksum = true);
size_t estimate_compressed_size(size_t uncompressed_size, int compression_level);
Status validate_config(const CompressionConfig &config);
void apply_level_parameters(CompressionConfig &config);
u32 get_optimal_block_size(u32 input_size, u32 compression_level);

constexpr const char *get_format_name() { return "cuda_zstd"; }
constexpr u32 get_format_version() { return 0x00010000; }
// reference include/cuda_zstd_manager.h:415-419 (skips leading skippable frames)
bool is_nvcomp_zstd_format(const void *compressed_data, size_t compressed_size);
Status extract_metadata(const void *compressed_data, size_t compressed_size, NvcompMetadata &metadata);
// 16-byte skippable metadata frame (reference SkippableFrameHeader + CustomMetadataFrame,
// src/cuda_zstd_manager.cu:309-318, 391-412) written to a host or device buffer
Status write_metadata_frame(void *output, size_t capacity, int compression_level, size_t *written, hipStream_t stream = 0);

}  // namespace cuda_zstd
#endif  // __cplusplus
#endif  // CUDA_ZSTD_MANAGER_H_

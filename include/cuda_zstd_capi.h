/*
 * cuda_zstd_capi.h — the C ABI of libcuda_zstd_hip.so (plain C, for cgo/ctypes/JNI).
 *
 * Every entry point keeps the reference's name, argument order and error
 * behaviour; only cudaStream_t became hipStream_t (same pointer ABI).
 *
 *  manager API   reference include/cuda_zstd_manager.h:433-479, src/cuda_zstd_c_api.cpp:10-209
 *  nvCOMP v5 API reference include/cuda_zstd_nvcomp.h:272-336, src/cuda_zstd_nvcomp.cpp:766-840
 *  hybrid API    reference include/cuda_zstd_hybrid.h:292-363
 *  batch API     NEW C counterparts of ZstdBatchManager::compress_batch
 *                (include/cuda_zstd_manager.h:148-150) and NvcompV5BatchManager::compress_async
 *                (include/cuda_zstd_nvcomp.h:112-121), which the reference exposes only in C++,
 *                plus one stream-ordered device-array entry (nvcomp_zstd_batched_compress_async_v5).
 *
 * Return codes of the int-returning functions are the reference's
 * status_to_nvcomp_error mapping (src/cuda_zstd_nvcomp.cpp:75-96):
 * 0 OK, 2 invalid parameter, 3 out of memory, 4 device error, 6 corrupt data,
 * 7 buffer too small, 10 checksum, 12 compression, everything else 1.
 */
#ifndef CUDA_ZSTD_CAPI_H_
#define CUDA_ZSTD_CAPI_H_

#include <hip/hip_runtime_api.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------- manager API (reference include/cuda_zstd_manager.h:437-475) ---------------- */
typedef struct cuda_zstd_manager_t cuda_zstd_manager_t;
typedef struct cuda_zstd_dict_t cuda_zstd_dict_t;

cuda_zstd_manager_t *cuda_zstd_create_manager(int compression_level);
void cuda_zstd_destroy_manager(cuda_zstd_manager_t *manager);
int cuda_zstd_compress(cuda_zstd_manager_t *manager, const void *src, size_t src_size, void *dst, size_t *dst_size,
                       void *workspace, size_t workspace_size, hipStream_t stream);
int cuda_zstd_decompress(cuda_zstd_manager_t *manager, const void *src, size_t src_size, void *dst, size_t *dst_size,
                         void *workspace, size_t workspace_size, hipStream_t stream);
size_t cuda_zstd_get_compress_workspace_size(cuda_zstd_manager_t *manager, size_t src_size);
size_t cuda_zstd_get_decompress_workspace_size(cuda_zstd_manager_t *manager, size_t compressed_size);
cuda_zstd_dict_t *cuda_zstd_train_dictionary(const void **samples, const size_t *sample_sizes, size_t num_samples, size_t dict_size);
/* host trainer with explicit COVER parameters (0 = default k 1024 / d 8); otherwise cuda_zstd_train_dictionary */
cuda_zstd_dict_t *cuda_zstd_train_dictionary_params(const void **samples, const size_t *sample_sizes, size_t num_samples,
                                                    size_t dict_size, unsigned k, unsigned d);
/* device trainer: d_samples = the samples back to back in device memory, sample_sizes a HOST array
 * (zero sizes allowed).  Stream-ordered on `stream` for its reads of d_samples; blocking on return
 * (the handle holds host bytes).  *dict_out = a handle whose content equals the host trainer's
 * for the same samples, or NULL.  Returns 0; 2 for bad arguments, a dict_size outside 256 B ..
 * 128 KiB, k > 65535 or 2^32 - 64 or more sample bytes; 7 when temp_bytes is below what
 * _get_temp_size reports (nothing is launched); 12 when training gave fewer than 256 bytes
 * (where the host entry returns NULL); 4 on a HIP error.  Window scores are kept in 64 bits, so
 * num_samples * k is not limited. */
size_t cuda_zstd_train_dictionary_device_get_temp_size(size_t total_sample_bytes, size_t num_samples, size_t dict_size, unsigned k);
int cuda_zstd_train_dictionary_device(const void *d_samples, const size_t *sample_sizes, size_t num_samples, size_t dict_size,
                                      unsigned k, unsigned d, void *d_temp, size_t temp_bytes, hipStream_t stream,
                                      cuda_zstd_dict_t **dict_out);
/* device trainer, one dictionary per group of samples in one call: d_samples = all samples back to
 * back in device memory, sample_sizes a HOST array (zero sizes allowed), group_counts a HOST array
 * of num_groups counts of consecutive samples (0 allowed) that sum to num_samples; 1 <= num_groups
 * <= 4096, what a dictionary set holds.  dict_size, k and d are common to the call, with the
 * single entry's limits: 256 B .. 128 KiB, k <= 65535 and fewer than 2^32 - 64 sample bytes PER
 * CALL (positions are 32-bit): a caller with more data calls twice.  Stream-ordered on `stream`
 * for its reads of d_samples; blocking on return (the handles hold host bytes).
 * dicts_out[g] = a raw-content handle whose bytes equal the host trainer's for group g's samples
 * alone, or NULL; group_status (optional) gets 0, or 12 where the group gave fewer than 256 bytes
 * (no samples, no bytes, fewer than k bytes).  A failed group does not affect its neighbours.
 * Returns 0 when the arguments were valid, whatever the groups report; 2 for a NULL required
 * pointer, no samples or no sample bytes at all, counts that do not sum to num_samples, num_groups
 * outside 1 .. 4096, or the limits above; 7 when temp_bytes is below what _get_temp_size reports
 * for the same arrays (nothing is launched); 4 on a HIP error.  Whenever it does not return 0,
 * every dicts_out[g] is NULL.  At most 64 groups are in flight (each with a 4 MiB frequency table
 * in d_temp, so the temp size stops growing with num_groups there); more groups run as successive
 * waves inside the call.  _get_temp_size returns 0 for arguments the call answers with 2. */
size_t cuda_zstd_train_dictionaries_device_get_temp_size(const size_t *sample_sizes, size_t num_samples, const size_t *group_counts,
                                                         size_t num_groups, size_t dict_size, unsigned k);
int cuda_zstd_train_dictionaries_device(const void *d_samples, const size_t *sample_sizes, size_t num_samples, const size_t *group_counts,
                                        size_t num_groups, size_t dict_size, unsigned k, unsigned d, void *d_temp, size_t temp_bytes,
                                        hipStream_t stream, cuda_zstd_dict_t **dicts_out, int *group_status);
/* dictionary::finalize_dictionary: the content of `content` (raw, or a formatted dictionary's) plus
 * entropy tables gathered by compressing the samples (an array of num_samples host or device
 * pointers) against it at `level` on the device -> a new formatted dictionary handle in *dict_out
 * (Dictionary_ID dict_id, or libzstd's hash rule when 0).  Use it with cuda_zstd_set_dict_entropy. */
int cuda_zstd_finalize_dictionary(const cuda_zstd_dict_t *content, const void *const *samples, const size_t *sample_sizes, size_t num_samples,
                                  int level, unsigned dict_id, hipStream_t stream, cuda_zstd_dict_t **dict_out);
void cuda_zstd_destroy_dictionary(cuda_zstd_dict_t *dict);
int cuda_zstd_set_dictionary(cuda_zstd_manager_t *manager, cuda_zstd_dict_t *dict);
/* dictionaries: cuda_zstd_train_dictionary is COVER training (raw content);
 * load = raw content or a formatted RFC 8878 §5 dictionary from a host buffer (reference
 * DictionaryManager::load_dictionary, include/cuda_zstd_dictionary.h:292); content copies the
 * bytes out (returns the size); layout gives the Dictionary_ID and content offset (0, 0 for raw).
 * Both return NULL for a dictionary outside 256 B .. 128 KiB (MIN/MAX_DICT_SIZE, the limits
 * cuda_zstd_set_dictionary enforces), so every handle they return can be set on a manager */
cuda_zstd_dict_t *cuda_zstd_load_dictionary(const void *buffer, size_t size);
size_t cuda_zstd_get_dictionary_content(const cuda_zstd_dict_t *dict, void *out, size_t capacity);
int cuda_zstd_get_dictionary_layout(const cuda_zstd_dict_t *dict, unsigned int *dict_id, size_t *content_offset);
int cuda_zstd_clear_dictionary(cuda_zstd_manager_t *manager);
const char *cuda_zstd_get_error_string(int error_code);
int cuda_zstd_is_error(int code);

/* batch (C counterpart of ZstdBatchManager::compress_batch, src/cuda_zstd_manager.cu:5715-5797).
 * Host arrays of device pointers; out_sizes[i] is capacity on entry, bytes on exit;
 * statuses (optional) receives each item's nvcomp-style code.  Blocking, like the reference. */
size_t cuda_zstd_get_batch_compress_workspace_size(cuda_zstd_manager_t *manager, const size_t *input_sizes, size_t count);
int cuda_zstd_compress_batch(cuda_zstd_manager_t *manager, const void *const *input_ptrs, const size_t *input_sizes, size_t count,
                             void *const *output_ptrs, size_t *output_sizes, int *statuses, void *workspace,
                             size_t workspace_size, hipStream_t stream);
size_t cuda_zstd_get_max_compressed_size(cuda_zstd_manager_t *manager, size_t src_size);
/* batch decompression (C counterpart of ZstdBatchManager::decompress_batch,
 * reference include/cuda_zstd_manager.h:153-158, src/cuda_zstd_manager.cu:5799-5885): the GPU
 * decoder, one launch for all items; out_sizes[i] capacity in, bytes out (0 on error). */
size_t cuda_zstd_get_batch_decompress_workspace_size(cuda_zstd_manager_t *manager, const size_t *compressed_sizes, size_t count);
int cuda_zstd_decompress_batch(cuda_zstd_manager_t *manager, const void *const *input_ptrs, const size_t *input_sizes, size_t count,
                               void *const *output_ptrs, size_t *output_sizes, int *statuses, void *workspace, size_t workspace_size,
                               hipStream_t stream);

/* ---------------- nvCOMP v5 API (reference include/cuda_zstd_nvcomp.h:277-331) ---------------- */
typedef void *nvcompZstdManagerHandle;
nvcompZstdManagerHandle nvcomp_zstd_create_manager_v5(int compression_level);
void nvcomp_zstd_destroy_manager_v5(nvcompZstdManagerHandle handle);
int nvcomp_zstd_compress_async_v5(nvcompZstdManagerHandle handle, const void *d_uncompressed, size_t uncompressed_size,
                                  void *d_compressed, size_t *compressed_size, void *d_temp, size_t temp_size, hipStream_t stream);
int nvcomp_zstd_decompress_async_v5(nvcompZstdManagerHandle handle, const void *d_compressed, size_t compressed_size,
                                    void *d_uncompressed, size_t *uncompressed_size, void *d_temp, size_t temp_size,
                                    hipStream_t stream);
size_t nvcomp_zstd_get_compress_temp_size_v5(nvcompZstdManagerHandle handle, size_t uncompressed_size);
size_t nvcomp_zstd_get_decompress_temp_size_v5(nvcompZstdManagerHandle handle, size_t compressed_size);

/* NvcompV5BatchManager as a C handle (reference include/cuda_zstd_nvcomp.h:85-137,
 * src/cuda_zstd_nvcomp.cpp:300-484).  Pointer and size arrays may live on the host or
 * the device (probed like the reference); blocking on return. */
typedef struct nvcomp_zstd_batch_manager_t nvcomp_zstd_batch_manager_t;
nvcomp_zstd_batch_manager_t *nvcomp_zstd_batch_create_v5(int compression_level, unsigned int chunk_size, int enable_checksum);
void nvcomp_zstd_batch_destroy_v5(nvcomp_zstd_batch_manager_t *mgr);
size_t nvcomp_zstd_batch_get_compress_temp_size_v5(nvcomp_zstd_batch_manager_t *mgr, const size_t *chunk_sizes, size_t num_chunks);
size_t nvcomp_zstd_batch_get_max_compressed_chunk_size_v5(nvcomp_zstd_batch_manager_t *mgr, size_t uncompressed_chunk_size);
int nvcomp_zstd_batch_compress_async_v5(nvcomp_zstd_batch_manager_t *mgr, const void *const *d_uncompressed_ptrs,
                                        const size_t *uncompressed_sizes, size_t num_chunks, void *const *d_compressed_ptrs,
                                        size_t *compressed_sizes, void *d_temp_storage, size_t temp_storage_bytes,
                                        hipStream_t stream);

/* Stream-ordered batched compression (nvCOMP nvcompBatchedZstdCompressAsync shape).
 * All arrays are DEVICE arrays; nothing is synchronised; results are valid once
 * `stream` reaches this point.  d_compressed_sizes[i] receives bytes written;
 * d_statuses[i] (optional) the item's nvcomp-style code.  Every chunk must be
 * <= max_uncompressed_chunk_bytes and every output buffer must hold
 * nvcomp_zstd_batch_get_max_compressed_chunk_size_v5(max_uncompressed_chunk_bytes). */
size_t nvcomp_zstd_batched_compress_get_temp_size_v5(size_t num_chunks, size_t max_uncompressed_chunk_bytes);
/* The same for the handle's level and dictionary (levels >= 5, ZH_DEEP_LEVEL, add the deep
 * matcher's scratch slots; a dictionary over 32 KiB chunks adds history blocks): what a handle at
 * its level, with or without a dictionary, needs for nvcomp_zstd_batched_compress_async_v5.  (The
 * static size above covers levels below 5 without a dictionary; at levels >= 5, or with a
 * dictionary, a workspace of that size fails loudly with 7 and nothing is launched.) */
size_t nvcomp_zstd_batch_get_batched_temp_size_v5(nvcomp_zstd_batch_manager_t *mgr, size_t num_chunks, size_t max_uncompressed_chunk_bytes);
/* A dictionary for the batch handle's compress/decompress calls (the C++
 * manager's set_dictionary).  With a dictionary, chunks over 32 KiB take two history blocks:
 * size the workspace with nvcomp_zstd_batch_get_batched_temp_size_v5 after setting it. */
int nvcomp_zstd_batch_set_dictionary_v5(nvcomp_zstd_batch_manager_t *mgr, cuda_zstd_dict_t *dict);
/* cuda_zstd_set_dict_entropy for a batch manager (both batch compress entries) */
int nvcomp_zstd_batch_set_dict_entropy_v5(nvcomp_zstd_batch_manager_t *mgr, int enable);
int nvcomp_zstd_batched_compress_async_v5(nvcomp_zstd_batch_manager_t *mgr, const void *const *d_uncompressed_ptrs,
                                          const size_t *d_uncompressed_sizes, size_t max_uncompressed_chunk_bytes,
                                          size_t num_chunks, void *const *d_compressed_ptrs, size_t *d_compressed_sizes,
                                          int *d_statuses, void *d_temp_storage, size_t temp_storage_bytes,
                                          hipStream_t stream);

/* The same call at one level per chunk: d_levels[i] is chunk i's level, a DEVICE int array such as
 * the one cuda_zstd_adaptive_analyze_batch_async leaves behind, read on the device.  Stream-ordered
 * like the call above: every array is a device array, nothing is allocated, synchronised or copied
 * to the host.  Frame i is byte-identical to what a handle at level d_levels[i] writes for chunk i
 * through nvcomp_zstd_batched_compress_async_v5 with the same max_uncompressed_chunk_bytes.  The
 * handle's level is ignored; its checksum setting applies.  A level outside 1..22 gives that chunk
 * size 0 and status 2 and leaves its output buffer untouched; its neighbours are unaffected.
 * Returns 2 for a null array, max_uncompressed_chunk_bytes == 0, a handle with a dictionary set or
 * more than 1,048,576 chunks (the one workgroup that ranks the chunks by level is kept to that),
 * 7 for a workspace below nvcomp_zstd_batched_compress_levels_get_temp_size_v5 (nothing is
 * launched); num_chunks == 0 succeeds and launches nothing.
 * Out of scope: dictionaries (a dictionary frame's block split depends on its level, so one block
 * count per chunk does not hold for the batch), dict_entropy, long-distance matching and the
 * streaming manager.
 * The workspace is that of a handle at a level >= 5 plus the chunks' ranks, one level byte per block
 * and the class ranges: at least what any dictionary-less handle needs for the call above. */
size_t nvcomp_zstd_batched_compress_levels_get_temp_size_v5(size_t num_chunks, size_t max_uncompressed_chunk_bytes);
int nvcomp_zstd_batched_compress_levels_async_v5(nvcomp_zstd_batch_manager_t *mgr, const void *const *d_uncompressed_ptrs,
                                                 const size_t *d_uncompressed_sizes, const int *d_levels,
                                                 size_t max_uncompressed_chunk_bytes, size_t num_chunks, void *const *d_compressed_ptrs,
                                                 size_t *d_compressed_sizes, int *d_statuses, void *d_temp_storage,
                                                 size_t temp_storage_bytes, hipStream_t stream);

/* The batched call with one prefix per chunk: d_prefix_ptrs[i] / d_prefix_sizes[i] (DEVICE arrays)
 * are the bytes that precede chunk i -- earlier data of its stream, the previous version of a shard
 * (zstd --patch-from per chunk), a per-tenant sample -- used as a raw-content dictionary.  Stream-
 * ordered like nvcomp_zstd_batched_compress_async_v5: every array is a device array, nothing is
 * allocated, synchronised or copied to the host.
 * Frame i is byte-identical to what ZstdBatchManager::compress_with_history(chunk i, prefix i) writes
 * at the handle's configuration; with d_prefix_sizes[i] == 0 it is the frame
 * nvcomp_zstd_batched_compress_async_v5 writes for chunk i.  The frames carry no Dictionary_ID and
 * decode with nvcomp_zstd_batched_decompress_prefix_async_v5 or libzstd's ZSTD_decompress_usingDict.
 * Only the tail of a prefix that the matcher stages is read.  Levels 1-4: the last 64 KiB - block
 * bytes; a chunk over 32 KiB is cut into 32 KiB blocks, the first sees the last 32 KiB of the prefix,
 * later blocks see the frame's previous 32 KiB.  Levels >= 5: the last 64 KiB.
 * A non-zero prefix size with a null pointer gives that chunk size 0 and status 2 and leaves its
 * output untouched; a chunk of size 0 behaves as in the plain entry; neighbours are unaffected.
 * Returns 2 for a null required array (d_statuses is optional), max_uncompressed_chunk_bytes == 0 or
 * a handle with a dictionary set; 7 for a workspace below
 * nvcomp_zstd_batch_get_batched_prefix_temp_size_v5 (nothing is launched); num_chunks == 0 succeeds
 * and launches nothing.  The handle's checksum setting applies; dict_entropy and enable_ldm have no
 * effect here.
 * Out of scope: a prefix together with a handle dictionary; with per-chunk levels; with dict_entropy
 * or long-distance matching; staging the aligned region of a reference for blocks after the first --
 * at levels 1-4 a 64 KiB chunk's second block sees the frame's own first half, not the reference's
 * second half, so delta users below level 5 should use chunks of <= 32 KiB (lifting that needs an
 * offset bias through the matcher and the sequence stage).
 * The workspace is that of a handle with a dictionary at its level. */
size_t nvcomp_zstd_batch_get_batched_prefix_temp_size_v5(nvcomp_zstd_batch_manager_t *mgr, size_t num_chunks,
                                                         size_t max_uncompressed_chunk_bytes);
int nvcomp_zstd_batched_compress_prefix_async_v5(nvcomp_zstd_batch_manager_t *mgr, const void *const *d_uncompressed_ptrs,
                                                 const size_t *d_uncompressed_sizes, const void *const *d_prefix_ptrs,
                                                 const size_t *d_prefix_sizes, size_t max_uncompressed_chunk_bytes, size_t num_chunks,
                                                 void *const *d_compressed_ptrs, size_t *d_compressed_sizes, int *d_statuses,
                                                 void *d_temp_storage, size_t temp_storage_bytes, hipStream_t stream);

/* NvcompV5BatchManager::decompress_async as a C handle call (reference include/cuda_zstd_nvcomp.h:97-99,
 * 119-125): host or device arrays, uncompressed_sizes[i] capacity in, bytes out; blocking on return. */
size_t nvcomp_zstd_batch_get_decompress_temp_size_v5(nvcomp_zstd_batch_manager_t *mgr, const size_t *compressed_sizes, size_t num_chunks);
int nvcomp_zstd_batch_decompress_async_v5(nvcomp_zstd_batch_manager_t *mgr, const void *const *d_compressed_ptrs,
                                          const size_t *compressed_sizes, size_t num_chunks, void *const *d_uncompressed_ptrs,
                                          size_t *uncompressed_sizes, void *d_temp_storage, size_t temp_storage_bytes, hipStream_t stream);

/* Stream-ordered batched decompression (nvCOMP nvcompBatchedZstdDecompressAsync shape).
 * All arrays are DEVICE arrays; nothing is synchronised.  d_uncompressed_caps[i] = output
 * capacity (null: max_uncompressed_chunk_bytes for every chunk); d_actual_sizes[i] receives
 * the bytes produced (0 on error); d_statuses[i] (optional) the nvcomp-style code.
 * Decodes any RFC 8878 frame (concatenated and skippable frames included) whose blocks
 * regenerate at most min(128 KiB, max_uncompressed_chunk_bytes) bytes of literals. */
size_t nvcomp_zstd_batched_decompress_get_temp_size_v5(size_t num_chunks, size_t max_uncompressed_chunk_bytes);
int nvcomp_zstd_batched_decompress_async_v5(nvcomp_zstd_batch_manager_t *mgr, const void *const *d_compressed_ptrs,
                                            const size_t *d_compressed_sizes, const size_t *d_uncompressed_caps,
                                            size_t max_uncompressed_chunk_bytes, size_t num_chunks, void *const *d_uncompressed_ptrs,
                                            size_t *d_actual_sizes, int *d_statuses, void *d_temp_storage, size_t temp_storage_bytes,
                                            hipStream_t stream);

/* The same call with one prefix per buffer (DEVICE arrays; size 0 or a null pointer: none): the
 * whole prefix is addressable in front of buffer i's frames, as with libzstd's
 * ZSTD_decompress_usingDict on raw content.  A frame that names a Dictionary_ID gets the
 * dictionary-wrong code (there is no formatted dictionary on this route).  The workspace is
 * nvcomp_zstd_batched_decompress_get_temp_size_v5; a handle with a dictionary set returns 2.
 * Out of scope: a prefix together with a handle dictionary. */
int nvcomp_zstd_batched_decompress_prefix_async_v5(nvcomp_zstd_batch_manager_t *mgr, const void *const *d_compressed_ptrs,
                                                   const size_t *d_compressed_sizes, const void *const *d_prefix_ptrs,
                                                   const size_t *d_prefix_sizes, const size_t *d_uncompressed_caps,
                                                   size_t max_uncompressed_chunk_bytes, size_t num_chunks, void *const *d_uncompressed_ptrs,
                                                   size_t *d_actual_sizes, int *d_statuses, void *d_temp_storage,
                                                   size_t temp_storage_bytes, hipStream_t stream);

/* A set of dictionaries on the device, for batches whose chunks use different dictionaries (one per
 * table, tenant, column or schema version).  Created from n = 1 .. 4,096 handles (raw content or
 * formatted, 256 B .. 128 KiB, as nvcomp_zstd_batch_set_dictionary_v5 accepts); the bytes are
 * copied, so the handles may be destroyed afterwards, and the set is immutable.  One device
 * allocation holds, per entry, what set_dictionary builds for one dictionary (the matchers' tables
 * of its content; for a formatted dictionary the encoder's view of its entropy section): about
 * 0.5 MiB per 64 KiB dictionary.  Two entries with the same non-zero Dictionary_ID are refused with
 * 2; raw-content entries (ID 0) are allowed and reachable by index only.  create blocks until the
 * tables are built (a constant number of launches per 64 dictionaries); destroy waits for the
 * stream-ordered calls that read the set.  find: the entry index of a non-zero Dictionary_ID, or -1. */
typedef struct cuda_zstd_dict_set_t cuda_zstd_dict_set_t;
int cuda_zstd_dict_set_create(const cuda_zstd_dict_t *const *dicts, size_t n, hipStream_t stream, cuda_zstd_dict_set_t **out);
void cuda_zstd_dict_set_destroy(cuda_zstd_dict_set_t *set);
size_t cuda_zstd_dict_set_count(const cuda_zstd_dict_set_t *set);
int cuda_zstd_dict_set_find(const cuda_zstd_dict_set_t *set, unsigned int dict_id);
/* Binds a set to the batch handle (null clears) for the two entries below and for
 * nvcomp_zstd_batched_decompress_async_v5 / nvcomp_zstd_batched_get_decompress_size_async_v5, which
 * then resolve every frame's dictionary from its Dictionary_ID on the device.  The handle keeps the
 * set's device memory alive while bound.  Not together with nvcomp_zstd_batch_set_dictionary_v5:
 * either call while the other is in place returns 2. */
int nvcomp_zstd_batch_set_dictionary_set_v5(nvcomp_zstd_batch_manager_t *mgr, cuda_zstd_dict_set_t *set);
/* The batched call with one dictionary per chunk: d_dict_index[i] (a DEVICE int32 array, read only
 * on the device) names chunk i's entry of the bound set, -1 none.  Stream-ordered like
 * nvcomp_zstd_batched_compress_async_v5: nothing is allocated, synchronised or copied to the host,
 * and the launches are the same whatever the set's size or the mix.
 * Frame i is byte-identical to what a handle at the same level, checksum and dict_entropy setting
 * with that one dictionary set writes for chunk i through nvcomp_zstd_batched_compress_async_v5: it
 * carries the entry's Dictionary_ID, its first block starts from the entry's precomputed tables and,
 * with dict_entropy, may use the entry's entropy section.  Index -1 gives the frame of a handle
 * without a dictionary.  An index below -1 or past the set gives that chunk size 0 and status 2 and
 * leaves its output untouched; neighbours are unaffected.
 * Returns 2 for a handle without a bound set, a null required array (d_statuses is optional),
 * max_uncompressed_chunk_bytes == 0 or enable_ldm; 7 for a workspace below
 * nvcomp_zstd_batch_get_batched_dicts_temp_size_v5 (nothing is launched); num_chunks == 0 succeeds.
 * Out of scope: a set together with per-chunk levels, with a per-chunk prefix, with long-distance
 * matching, and the streaming managers.
 * The workspace is nvcomp_zstd_batch_get_batched_prefix_temp_size_v5's. */
size_t nvcomp_zstd_batch_get_batched_dicts_temp_size_v5(nvcomp_zstd_batch_manager_t *mgr, size_t num_chunks,
                                                        size_t max_uncompressed_chunk_bytes);
int nvcomp_zstd_batched_compress_dicts_async_v5(nvcomp_zstd_batch_manager_t *mgr, const void *const *d_uncompressed_ptrs,
                                                const size_t *d_uncompressed_sizes, const int32_t *d_dict_index,
                                                size_t max_uncompressed_chunk_bytes, size_t num_chunks, void *const *d_compressed_ptrs,
                                                size_t *d_compressed_sizes, int *d_statuses, void *d_temp_storage,
                                                size_t temp_storage_bytes, hipStream_t stream);
/* nvcomp_zstd_batched_decompress_async_v5 with an entry index per buffer (a DEVICE int32 array, or
 * null): -1 or null resolves every frame by its Dictionary_ID, an index >= 0 uses that entry (how a
 * raw-content entry, whose frames carry no ID, is named), an index outside the set gives the buffer
 * status 2.  Per frame: a non-zero ID that is not in the set, or that differs from the named
 * entry's, gets the dictionary-wrong code; a frame without an ID and without an index is decoded
 * without a dictionary; with an index the entry's content precedes it and a formatted entry's
 * tables and repcodes seed it.  Same workspace as the plain entry; 2 without a bound set. */
int nvcomp_zstd_batched_decompress_dicts_async_v5(nvcomp_zstd_batch_manager_t *mgr, const void *const *d_compressed_ptrs,
                                                  const size_t *d_compressed_sizes, const int32_t *d_dict_index,
                                                  const size_t *d_uncompressed_caps, size_t max_uncompressed_chunk_bytes, size_t num_chunks,
                                                  void *const *d_uncompressed_ptrs, size_t *d_actual_sizes, int *d_statuses,
                                                  void *d_temp_storage, size_t temp_storage_bytes, hipStream_t stream);

/* Many streams in one call: num_streams streams, each with a device-resident window of its last
 * 64 KiB, compressed or decoded one chunk per stream per call.  create allocates everything the
 * object owns (the compress and decode workspaces, one pair of 64 KiB window buffers per stream and
 * direction, the prefix pointer and size arrays); a call allocates nothing and synchronises nothing.
 * All arrays are DEVICE arrays of num_streams entries.
 * compress_async: chunk i of stream i goes through nvcomp_zstd_batched_compress_prefix_async_v5
 * behind window i, then one launch (zh_window_update_kernel, one workgroup per stream) advances every
 * window.  Frame i is what ZstdStreamingManager::compress_chunk_with_history writes for that stream.
 * Every output buffer holds cuda_zstd_stream_batch_max_compressed_chunk_size bytes.
 * decompress_async: the same with nvcomp_zstd_batched_decompress_prefix_async_v5 and the decoded
 * output (d_out_caps null: max_chunk_bytes for every stream).  Frames decode in stream order.
 * A stream whose item did not succeed keeps its window; an idle stream (d_in_sizes[i] == 0) reports
 * size 0 and status 2 like any empty item and keeps its window.  d_statuses is optional.
 * reset: every window of both directions empty again (stream-ordered).
 * Returns 2 for a null handle or required array, otherwise as the batched entries.
 * Out of scope: dictionaries, per-chunk levels, dict_entropy, long-distance matching. */
typedef struct cuda_zstd_stream_batch_t cuda_zstd_stream_batch_t;
cuda_zstd_stream_batch_t *cuda_zstd_stream_batch_create(int level, size_t num_streams, size_t max_chunk_bytes);
void cuda_zstd_stream_batch_destroy(cuda_zstd_stream_batch_t *sb);
size_t cuda_zstd_stream_batch_max_compressed_chunk_size(cuda_zstd_stream_batch_t *sb);
int cuda_zstd_stream_batch_compress_async(cuda_zstd_stream_batch_t *sb, const void *const *d_in_ptrs, const size_t *d_in_sizes,
                                          void *const *d_out_ptrs, size_t *d_out_sizes, int *d_statuses, hipStream_t stream);
int cuda_zstd_stream_batch_decompress_async(cuda_zstd_stream_batch_t *sb, const void *const *d_in_ptrs, const size_t *d_in_sizes,
                                            const size_t *d_out_caps, void *const *d_out_ptrs, size_t *d_out_sizes, int *d_statuses,
                                            hipStream_t stream);
int cuda_zstd_stream_batch_reset(cuda_zstd_stream_batch_t *sb, hipStream_t stream);

/* Batched decompressed-size query on the device (nvCOMP nvcompBatchedZstdGetDecompressSizeAsync
 * shape).  All arrays are DEVICE arrays; one launch; nothing is synchronised or allocated and no
 * workspace is needed; num_chunks / count == 0 succeeds and launches nothing.
 * d_uncompressed_bytes[i] receives the bytes that all frames of buffer i regenerate (skippable frames
 * skipped): a frame's Frame_Content_Size where present (believed, as ZSTD_findDecompressedSize
 * does; a decode rejects a frame whose field lies), otherwise the sum over its blocks, found by
 * reading the sequence bitstreams without decoding anything -- exact for frames of streaming
 * writers, which carry no size.  For every buffer the decoder accepts, the size is exactly what it
 * produces.  d_statuses (optional, may be NULL) receives per buffer the code a decode reports: the
 * nvcomp-style code (the _v5 entry) or the cuda_zstd status value (the manager entry); 2 for an empty
 * or null buffer; the size is 0 wherever the status is not 0.  The handle's dictionary, if set,
 * is used as by the batched decompress entry. */
int nvcomp_zstd_batched_get_decompress_size_async_v5(nvcomp_zstd_batch_manager_t *mgr, const void *const *d_compressed_ptrs,
                                                     const size_t *d_compressed_bytes, size_t *d_uncompressed_bytes, int *d_statuses,
                                                     size_t num_chunks, hipStream_t stream);
int cuda_zstd_get_decompressed_sizes_async(cuda_zstd_manager_t *manager, const void *const *d_ptrs, const size_t *d_sizes, size_t count,
                                           size_t *d_out_sizes, int *d_statuses, hipStream_t stream);

/* ---------------- hybrid API (reference include/cuda_zstd_hybrid.h:296-359) ---------------- */
typedef struct cuda_zstd_hybrid_engine_t cuda_zstd_hybrid_engine_t;
typedef struct {
  unsigned int mode;
  size_t cpu_size_threshold;
  size_t gpu_device_threshold;
  int compression_level;
  int enable_profiling;
  unsigned int cpu_thread_count;
} cuda_zstd_hybrid_config_t;
typedef struct {
  unsigned int backend_used;
  unsigned int input_location;
  unsigned int output_location;
  double total_time_ms;
  double transfer_time_ms;
  double compute_time_ms;
  double throughput_mbps;
  size_t input_bytes;
  size_t output_bytes;
  float compression_ratio;
} cuda_zstd_hybrid_result_t;
cuda_zstd_hybrid_engine_t *cuda_zstd_hybrid_create(const cuda_zstd_hybrid_config_t *config);
cuda_zstd_hybrid_engine_t *cuda_zstd_hybrid_create_default(void);
void cuda_zstd_hybrid_destroy(cuda_zstd_hybrid_engine_t *engine);
int cuda_zstd_hybrid_compress(cuda_zstd_hybrid_engine_t *engine, const void *input, size_t input_size, void *output,
                              size_t *output_size, unsigned int input_loc, unsigned int output_loc,
                              cuda_zstd_hybrid_result_t *result, hipStream_t stream);
int cuda_zstd_hybrid_decompress(cuda_zstd_hybrid_engine_t *engine, const void *input, size_t input_size, void *output,
                                size_t *output_size, unsigned int input_loc, unsigned int output_loc,
                                cuda_zstd_hybrid_result_t *result, hipStream_t stream);
size_t cuda_zstd_hybrid_max_compressed_size(cuda_zstd_hybrid_engine_t *engine, size_t input_size);
unsigned int cuda_zstd_hybrid_query_routing(cuda_zstd_hybrid_engine_t *engine, size_t data_size, unsigned int input_loc,
                                            unsigned int output_loc, int is_compression);

/* ---------------- streaming (reference ZstdStreamingManager, include/cuda_zstd_manager.h:300-352) ----
 * No C binding in the reference; added so the streaming path is reachable from C/ctypes.  Every
 * chunk is a complete frame; with_history = compress_chunk_with_history (the preceding <= 64 KiB
 * of the stream as raw-content history); decompress_chunk keeps the decoded window, so chunks
 * decode in stream order.  Device buffers; blocking on return. */
typedef struct cuda_zstd_stream_t cuda_zstd_stream_t;
cuda_zstd_stream_t *cuda_zstd_stream_create(int compression_level);
void cuda_zstd_stream_destroy(cuda_zstd_stream_t *s);
int cuda_zstd_stream_compress_chunk(cuda_zstd_stream_t *s, const void *src, size_t src_size, void *dst, size_t *dst_size, int with_history,
                                    int is_last_chunk, hipStream_t stream);
int cuda_zstd_stream_decompress_chunk(cuda_zstd_stream_t *s, const void *src, size_t src_size, void *dst, size_t *dst_size,
                                      int *is_last_chunk, hipStream_t stream);
int cuda_zstd_stream_reset(cuda_zstd_stream_t *s);

/* ---------------- frame metadata (skippable frames) ----------------
 * A 16-byte skippable frame [0x184D2A50][8][0x444D5A43 "CZMD"][level] in front of frames: the
 * reference's SkippableFrameHeader + CustomMetadataFrame (src/cuda_zstd_manager.cu:309-318,
 * writer :391-412).  dst: host or device.  extract: the first zstd frame's header fields after
 * any skippable frames (reference extract_metadata, src/cuda_zstd_manager.cu:992-1030); level 3
 * when no metadata frame is present.  Return nvcomp-style codes. */
int cuda_zstd_write_metadata_frame(void *dst, size_t capacity, int compression_level, size_t *written, hipStream_t stream);
int cuda_zstd_extract_metadata(const void *src, size_t size, unsigned int *compression_level, unsigned long long *uncompressed_size,
                               unsigned int *dictionary_id, int *has_checksum);

/* ---------------- seekable streams ----------------
 * The Zstandard seekable format: frame_0 .. frame_{N-1}, then one skippable frame holding the
 * seek table (all little-endian):
 *   u32 0x184D2A5E | u32 Frame_Size = N*E + 9 | N x { u32 Compressed_Size; u32 Decompressed_Size;
 *   [u32 Checksum] } | u32 N | u8 descriptor (bit 7: checksums; bits 6..2 reserved, 0) | u32 0x8F92EAB1
 * E = 8 without checksums, 12 with; Checksum = low 32 bits of XXH64 (seed 0) of the frame's
 * decompressed bytes.  Stock zstd decoders decode the whole stream and skip the table.
 * Limits: N <= 0x8000000, each size field <= 0x40000000.
 *
 * pack_async: stream-ordered, every array a device array (what
 * nvcomp_zstd_batched_compress_async_v5 leaves behind plus the chunks' uncompressed sizes;
 * d_uncompressed_ptrs only with checksums).  *d_out_size = bytes of the stream and *d_status = 0,
 * or *d_out_size = 0 and *d_status = the first failing item's status, 2 for an item size of 0 or
 * over max_compressed_chunk_bytes or the format's limits, 7 when out_capacity is too small.
 * Nothing of d_out is written on failure, and nothing past *d_out_size on success.
 *
 * info: stream_buf in host or device memory; 6 for a damaged table.
 * read: decodes [offset, offset + length) of the stream's content into d_out through the batched
 * GPU decoder (with the handle's dictionary, if set); the table is parsed and validated on the
 * device.  Blocking.  *written (host) = length on success, else 0.  Codes: 2 a range past the
 * content (d_out untouched), 6 a damaged table, 7 a temp buffer too small (below the table-sized
 * part: nothing is launched; below the part sized by the frames the range covers: no decode is
 * launched), 10 a checksum mismatch with verify_checksums on a checksummed stream, or the first
 * failing frame's decoder code.  read_get_temp_size covers any range; _jobs covers ranges that
 * touch at most max_jobs frames with content.
 *
 * read_ranges: num_ranges ranges of the content in one call.  d_offsets, d_lengths, d_out_ptrs
 * and d_range_statuses are device arrays of num_ranges; the host never reads the first three.
 * The table is scanned once, every frame that a range touches is decoded once (into a staging
 * slot in d_temp) and range r's bytes are copied to d_out_ptrs[r].  Ranges may overlap, repeat
 * and come in any order; max_length bounds every length.  Blocking: one wait for the number of
 * frames to decode, one at the end.  The return value is the call's: 2 a bad argument, 6 a
 * damaged table, 7 a temp buffer below read_ranges_get_temp_size(num_frames, num_ranges, frames
 * the ranges touch, largest Decompressed_Size); then no status and no destination is written.
 * Otherwise 0, and d_range_statuses[r] = 0, or 2 for offset + length past the content or
 * length > max_length, or the code (a decoder code, 6 for a size that disagrees with the table,
 * 10 for a checksum mismatch with verify_checksums) of the lowest failing frame the range
 * touches; no byte of a failed range's destination is written.  A length of 0 is valid.
 * *frames_decoded (host, optional) = the number of frames decoded. */
size_t cuda_zstd_seekable_max_size(size_t num_frames, size_t max_compressed_chunk_bytes, int with_checksums);
size_t cuda_zstd_seekable_pack_get_temp_size(size_t num_frames);
int cuda_zstd_seekable_pack_async(const void *const *d_frame_ptrs, const size_t *d_frame_sizes, const int *d_frame_statuses,
                                  const void *const *d_uncompressed_ptrs, const size_t *d_uncompressed_sizes, size_t num_frames,
                                  size_t max_compressed_chunk_bytes, int with_checksums, void *d_out, size_t out_capacity, size_t *d_out_size,
                                  int *d_status, void *d_temp, size_t temp_bytes, hipStream_t stream);
int cuda_zstd_seekable_info(const void *stream_buf, size_t size, size_t *num_frames, unsigned long long *total_uncompressed,
                            unsigned int *max_frame_uncompressed, int *has_checksums);
size_t cuda_zstd_seekable_read_get_temp_size(size_t num_frames, size_t max_frame_uncompressed);
size_t cuda_zstd_seekable_read_get_temp_size_jobs(size_t num_frames, size_t max_jobs, size_t max_frame_uncompressed);
int cuda_zstd_seekable_read(nvcomp_zstd_batch_manager_t *mgr, const void *d_stream, size_t size, unsigned long long offset, size_t length,
                            void *d_out, size_t *written, int verify_checksums, void *d_temp, size_t temp_bytes, hipStream_t stream);
size_t cuda_zstd_seekable_read_ranges_get_temp_size(size_t num_frames, size_t num_ranges, size_t max_jobs, size_t max_frame_uncompressed);
int cuda_zstd_seekable_read_ranges(nvcomp_zstd_batch_manager_t *mgr, const void *d_stream, size_t size, const unsigned long long *d_offsets,
                                   const size_t *d_lengths, void *const *d_out_ptrs, size_t num_ranges, size_t max_length, int verify_checksums,
                                   int *d_range_statuses, size_t *frames_decoded, void *d_temp, size_t temp_bytes, hipStream_t stream);

/* ---------------- the seek table of concatenated frames that have none ----------------
 * index: finds the frames of d_stream (size bytes of Zstandard and skippable frames back to back:
 * pzstd output, joined .zst files, frames written one after another) on the device and writes the
 * seek table for them to d_table: one entry per frame, skippable frames included with a
 * Decompressed_Size of 0, descriptor 0 (no checksums).  A frame without a Frame_Content_Size gets
 * its exact size from the decoder's size pass, with the dictionary or dictionary set of `mgr` (may
 * be NULL: no dictionary).  d_table may be (char *)d_stream + size when the caller left room: the
 * size + *table_bytes bytes are then a seekable stream for every cuda_zstd_seekable_* call and for
 * stock zstd.  Blocking.  *table_bytes, *num_frames and *error_offset are host words, all required.
 * Codes: 0; 2 a null or empty stream, a null output pointer, or a frame beyond the format's limits
 * (more than 0x8000000 frames, a size over 0x40000000); 7 a temp buffer below
 * index_get_temp_size(size, max_frames) (nothing is launched), more than max_frames frames
 * (*num_frames = the stream's frame count, for a second call) or a table_capacity below
 * 17 + 8 * frames; 6 a malformed stream, 1 when the first four bytes are no magic (the decoder's
 * codes for the same bytes); or the size pass's code for the lowest frame it fails on (1 for a
 * dictionary that is missing or wrong).  On a malformed stream or a failed size *num_frames = the
 * complete frames before the failing one and *error_offset = its byte offset.  On every non-zero
 * return no byte of d_table is written, on success none past *table_bytes.
 * The frames are found speculatively: every position that spells a frame magic is a candidate, and
 * the temp buffer holds 2 * max_frames + 1024 of them (max_frames counts up to 0x8000000).  A stream
 * with more (frames nested in raw blocks or skippable payloads) is walked frame after frame by one
 * wave instead, with the same result.  index_get_temp_size: 0 for stream_bytes == 0.
 * cuda_zstd_hip_frames_index_path (test hook): 0 the choice above, 1 always the serial walker;
 * _last_path: which of the two the last call took (-1: no call has launched anything yet).
 * cuda_zstd_hip_frames_index_split (benchmark hook): on != 0 times the speculative path's kernels
 * with HIP events; ms (4 floats, optional) = the last such call's candidate write, span, reach and
 * collect milliseconds. */
size_t cuda_zstd_seekable_index_get_temp_size(size_t stream_bytes, size_t max_frames);
int cuda_zstd_seekable_index(nvcomp_zstd_batch_manager_t *mgr /* may be NULL */, const void *d_stream, size_t size, size_t max_frames,
                             void *d_table, size_t table_capacity, size_t *table_bytes, size_t *num_frames,
                             unsigned long long *error_offset, void *d_temp, size_t temp_bytes, hipStream_t stream);
void cuda_zstd_hip_frames_index_path(int path);
int cuda_zstd_hip_frames_index_last_path(void);
void cuda_zstd_hip_frames_index_split(int on, float *ms);

/* ---------------- adaptive level selection ----------------
 * C counterpart of include/cuda_zstd_adaptive.h (reference adaptive::AdaptiveLevelSelector), for
 * whole batches: which level a chunk is worth, from statistics of its first
 * min(size, sample_bytes) bytes -- byte histogram and entropy, equal neighbours, longest run
 * (saturating at 256), short-period pattern score -- and the reference's decision tree.
 * preference: 0 speed, 1 balanced, 2 ratio.
 *
 * analyze_batch_async: stream-ordered; d_ptrs, d_sizes, d_stats, d_levels and d_temp are DEVICE
 * arrays, nothing is allocated or synchronised, results are valid once `stream` reaches this
 * point.  d_levels[i] = the level of chunk i; d_stats[i] (d_stats may be NULL) its statistics.  A
 * chunk of size 0 gets all-zero statistics and level 3.  d_temp: 4-byte aligned,
 * cuda_zstd_adaptive_get_temp_size(num_chunks) bytes.  num_chunks == 0 does nothing.
 * select_level: one device buffer; waits for `stream` and fills *h_out (host).
 * finalize_host: the derived values and the level from integer statistics computed elsewhere
 * (the function the device uses); host only, needs no GPU.
 * Codes: 2 for a null pointer, a preference outside 0..2, sample_bytes == 0, select_level's
 * size == 0, a misaligned d_temp or a batch too large for one launch (num_chunks x 16 KiB tiles of
 * sample_bytes over 2^31 - 1); 7 for a short temp; 4 on a HIP error. */
typedef struct {
  unsigned sample_size, repeated_pairs, max_run_length, pattern_score, unique_bytes, flags; /* bit0 has_patterns, bit1 is_random */
  float entropy, repetition_ratio, compressibility;
  int level;
} cuda_zstd_adaptive_stats_t;
size_t cuda_zstd_adaptive_get_temp_size(size_t num_chunks);
int cuda_zstd_adaptive_analyze_batch_async(const void *const *d_ptrs, const size_t *d_sizes, size_t num_chunks, size_t sample_bytes,
                                           int preference, cuda_zstd_adaptive_stats_t *d_stats /* may be NULL */, int *d_levels,
                                           void *d_temp, size_t temp_bytes, hipStream_t stream);
int cuda_zstd_adaptive_select_level(const void *d_data, size_t size, size_t sample_bytes, int preference,
                                    cuda_zstd_adaptive_stats_t *h_out, hipStream_t stream);
int cuda_zstd_adaptive_finalize_host(const unsigned *hist256, unsigned sample_size, unsigned repeated_pairs, unsigned max_run_length,
                                     unsigned pattern_score, int preference, cuda_zstd_adaptive_stats_t *out);

/* ---------------- long-distance matching (INTEGRATION.md for what ignores it) ----------------
 * With it on, cuda_zstd_compress of one buffer of more than 64 KiB finds repeats further back than
 * the 64 KiB its block matcher sees (up to 2^window_log bytes, at most 2^29 - 4) and writes each as a
 * block of its own; cuda_zstd_get_compress_workspace_size grows accordingly (three block slots per
 * 32 KiB plus the table).  enable != 0: window_log / hash_log 0 select 27 / 20 (`zstd --long`).
 * enable == 0: matching off; a window_log / hash_log of 0 leaves the manager's value alone, another
 * value is stored, and frames and workspace sizes are what a manager with that window gives without
 * this feature.  Returns 2 for a window_log outside 16..31; the table size is clamped to
 * 2^10..2^30.  Batch, dictionary and streaming entry points ignore it. */
int cuda_zstd_set_long_distance(cuda_zstd_manager_t *manager, int enable, unsigned window_log, unsigned hash_log);
/* Use a formatted dictionary's entropy section when compressing (CompressionConfig::dict_entropy):
 * the first block of a frame starts from the dictionary's repcodes and may reuse its Huffman and
 * FSE tables (treeless literals, Repeat_Mode).  0 (the default): frames as before.  No effect
 * without a dictionary, with raw content, or on streaming-history frames. */
int cuda_zstd_set_dict_entropy(cuda_zstd_manager_t *manager, int enable);
/* Content checksum on the manager's frames (0: none, the default). */
int cuda_zstd_set_checksum(cuda_zstd_manager_t *manager, int enable);
/* Inspection: the finder's decision per 32 KiB cell of a device buffer, as cuda_zstd_compress would
 * take it: host_records[3 i .. 3 i + 2] = {seg_start, seg_len, distance} (seg_len 0: the cell is not
 * split).  capacity in records; workspace as for cuda_zstd_compress.  Returns the number of cells,
 * 0 when long-distance matching does not apply to the buffer (off, <= 64 KiB, a dictionary is
 * set, over 4 GiB), -1 on error. */
long long cuda_zstd_hip_ldm_plan(cuda_zstd_manager_t *manager, const void *d_src, size_t size, unsigned int *host_records, size_t capacity,
                                 void *workspace, size_t workspace_size, hipStream_t stream);
/* HIP events around the finder's two kernels: on != 0 starts recording; on == 0 stops and stores the
 * summed milliseconds of the launches since then in *ms (optional). */
void cuda_zstd_hip_ldm_profile(int on, double *ms);
/* The same around zh_window_update_kernel (cuda_zstd_stream_batch_*). */
void cuda_zstd_hip_window_profile(int on, double *ms);

/* ---------------- library info ---------------- */
const char *cuda_zstd_hip_version(void);
/* Per-kernel timing with HIP events recorded on the launch stream (bench.py roofline).
 * collect() waits for the recorded launches and returns their count; ms3[0..2] = summed
 * milliseconds of K1 (zh_lz_kernel), the entropy stage (zh_entropy_kernel +
 * zh_fse_chain_kernel + zh_seq_pack_kernel) and the frame tail (zh_gather_kernel +
 * zh_checksum_kernel). */
void cuda_zstd_hip_profile_enable(int on);
int cuda_zstd_hip_profile_collect(double *ms3);
/* on != 0: later cuda_zstd_train_dictionary_device calls time their kernel groups with HIP events;
 * ms3 (optional) receives the last such call's milliseconds: d-mer ids + frequencies, prevdist,
 * the epoch-step loop. */
void cuda_zstd_hip_dict_train_profile(int on, double *ms3);
/* LDS bytes requested by K1 (which = 0) and the entropy kernel (1), for launch-bound checks. */
unsigned int cuda_zstd_hip_kernel_lds_bytes(int which);

#ifdef __cplusplus
}
#endif
#endif /* CUDA_ZSTD_CAPI_H_ */

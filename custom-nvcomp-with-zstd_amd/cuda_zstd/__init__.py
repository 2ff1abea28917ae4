"""Python binding of libcuda_zstd_hip.so (gfx950 Zstandard compressor).

Mirrors the reference's Python package (python/cuda_zstd/__init__.py:90-120,
python/src/binding.cpp:151-976): ``Manager`` (compress / decompress /
compress_batch / decompress_batch), ``HybridEngine``, module-level ``compress``,
``decompress``, ``compress_batch``, ``decompress_batch``, ``hybrid_compress``,
``hybrid_decompress``, ``validate_compressed_data``, ``estimate_compressed_size``,
``is_cuda_available``, ``get_cuda_device_info`` and the level constants -- plus a
``StreamingManager``, the dictionary / batched device entries and adaptive level selection
(``analyze_batch``, ``select_level``, ``is_compressible``, ``compress_batch_adaptive``), all over the
library's C ABI (include/cuda_zstd_capi.h).  Host inputs (bytes, bytearray, numpy)
give host ``bytes`` back, as the reference's binding does; torch device tensors stay
on the device.  PyTorch is only used for device memory and streams.

The product path never falls back to a CPU implementation: if the shared
library or a GPU is missing, every call raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CUDA_ZSTD_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "libcuda_zstd_hip.so")

# nvcomp-style return codes (reference src/cuda_zstd_nvcomp.cpp:75-96)
OK, INVALID, OOM, DEVICE_ERROR, CORRUPT, TOO_SMALL, CHECKSUM, COMPRESSION = 0, 2, 3, 4, 6, 7, 10, 12

_lib = None


class ZstdError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        super().__init__(f"{what}: {error_string(code)} (code {code})")


def lib() -> ctypes.CDLL:
    """Load the HIP library (raises if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not found: build it with __graft_entry__.build() (make -C custom-nvcomp-with-zstd_amd)")
        # PyTorch brings its own HIP runtime.  Loaded after this library it is a second runtime in
        # the process, and the library's calls on torch's device pointers fail (HIP runtime error);
        # loaded first, the library binds to the same one.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        psz, pvp, pi = ctypes.POINTER(sz), ctypes.POINTER(vp), ctypes.POINTER(i)
        sig = {
            "cuda_zstd_create_manager": (vp, [i]),
            "cuda_zstd_destroy_manager": (None, [vp]),
            "cuda_zstd_compress": (i, [vp, vp, sz, vp, psz, vp, sz, vp]),
            "cuda_zstd_decompress": (i, [vp, vp, sz, vp, psz, vp, sz, vp]),
            "cuda_zstd_get_compress_workspace_size": (sz, [vp, sz]),
            "cuda_zstd_get_decompress_workspace_size": (sz, [vp, sz]),
            "cuda_zstd_get_max_compressed_size": (sz, [vp, sz]),
            "cuda_zstd_get_batch_compress_workspace_size": (sz, [vp, psz, sz]),
            "cuda_zstd_compress_batch": (i, [vp, pvp, psz, sz, pvp, psz, pi, vp, sz, vp]),
            "cuda_zstd_get_error_string": (ctypes.c_char_p, [i]),
            "cuda_zstd_is_error": (i, [i]),
            "cuda_zstd_train_dictionary": (vp, [pvp, psz, sz, sz]),
            "cuda_zstd_train_dictionary_params": (vp, [pvp, psz, sz, sz, ctypes.c_uint, ctypes.c_uint]),
            "cuda_zstd_train_dictionary_device_get_temp_size": (sz, [sz, sz, sz, ctypes.c_uint]),
            "cuda_zstd_train_dictionary_device": (i, [vp, psz, sz, sz, ctypes.c_uint, ctypes.c_uint, vp, sz, vp, pvp]),
            "cuda_zstd_train_dictionaries_device_get_temp_size": (sz, [psz, sz, psz, sz, sz, ctypes.c_uint]),
            "cuda_zstd_train_dictionaries_device": (i, [vp, psz, sz, psz, sz, sz, ctypes.c_uint, ctypes.c_uint, vp, sz, vp, pvp, pi]),
            "cuda_zstd_hip_dict_train_profile": (None, [i, ctypes.POINTER(ctypes.c_double)]),
            "cuda_zstd_load_dictionary": (vp, [vp, sz]),
            "cuda_zstd_finalize_dictionary": (i, [vp, pvp, psz, sz, i, ctypes.c_uint, vp, pvp]),
            "cuda_zstd_destroy_dictionary": (None, [vp]),
            "cuda_zstd_set_dictionary": (i, [vp, vp]),
            "cuda_zstd_clear_dictionary": (i, [vp]),
            "cuda_zstd_get_dictionary_content": (sz, [vp, vp, sz]),
            "cuda_zstd_get_dictionary_layout": (i, [vp, ctypes.POINTER(ctypes.c_uint), psz]),
            "nvcomp_zstd_batch_create_v5": (vp, [i, ctypes.c_uint, i]),
            "nvcomp_zstd_batch_destroy_v5": (None, [vp]),
            "nvcomp_zstd_batch_get_compress_temp_size_v5": (sz, [vp, psz, sz]),
            "nvcomp_zstd_batch_get_max_compressed_chunk_size_v5": (sz, [vp, sz]),
            "nvcomp_zstd_batch_compress_async_v5": (i, [vp, vp, vp, sz, vp, vp, vp, sz, vp]),
            "nvcomp_zstd_batched_compress_get_temp_size_v5": (sz, [sz, sz]),
            "nvcomp_zstd_batch_get_batched_temp_size_v5": (sz, [vp, sz, sz]),
            "nvcomp_zstd_batch_set_dictionary_v5": (i, [vp, vp]),
            "nvcomp_zstd_batched_compress_async_v5": (i, [vp, vp, vp, sz, sz, vp, vp, vp, vp, sz, vp]),
            "nvcomp_zstd_batched_compress_levels_get_temp_size_v5": (sz, [sz, sz]),
            "nvcomp_zstd_batched_compress_levels_async_v5": (i, [vp, vp, vp, vp, sz, sz, vp, vp, vp, vp, sz, vp]),
            "nvcomp_zstd_batch_get_batched_prefix_temp_size_v5": (sz, [vp, sz, sz]),
            "nvcomp_zstd_batched_compress_prefix_async_v5": (i, [vp, vp, vp, vp, vp, sz, sz, vp, vp, vp, vp, sz, vp]),
            "nvcomp_zstd_batched_decompress_prefix_async_v5": (i, [vp, vp, vp, vp, vp, vp, sz, sz, vp, vp, vp, vp, sz, vp]),
            "cuda_zstd_dict_set_create": (i, [pvp, sz, vp, pvp]),
            "cuda_zstd_dict_set_destroy": (None, [vp]),
            "cuda_zstd_dict_set_count": (sz, [vp]),
            "cuda_zstd_dict_set_find": (i, [vp, ctypes.c_uint]),
            "nvcomp_zstd_batch_set_dictionary_set_v5": (i, [vp, vp]),
            "nvcomp_zstd_batch_get_batched_dicts_temp_size_v5": (sz, [vp, sz, sz]),
            "nvcomp_zstd_batched_compress_dicts_async_v5": (i, [vp, vp, vp, vp, sz, sz, vp, vp, vp, vp, sz, vp]),
            "nvcomp_zstd_batched_decompress_dicts_async_v5": (i, [vp, vp, vp, vp, vp, sz, sz, vp, vp, vp, vp, sz, vp]),
            "cuda_zstd_stream_batch_create": (vp, [i, sz, sz]),
            "cuda_zstd_stream_batch_destroy": (None, [vp]),
            "cuda_zstd_stream_batch_max_compressed_chunk_size": (sz, [vp]),
            "cuda_zstd_stream_batch_compress_async": (i, [vp, vp, vp, vp, vp, vp, vp]),
            "cuda_zstd_stream_batch_decompress_async": (i, [vp, vp, vp, vp, vp, vp, vp, vp]),
            "cuda_zstd_stream_batch_reset": (i, [vp, vp]),
            "cuda_zstd_get_batch_decompress_workspace_size": (sz, [vp, psz, sz]),
            "cuda_zstd_decompress_batch": (i, [vp, pvp, psz, sz, pvp, psz, pi, vp, sz, vp]),
            "nvcomp_zstd_batch_get_decompress_temp_size_v5": (sz, [vp, psz, sz]),
            "nvcomp_zstd_batch_decompress_async_v5": (i, [vp, vp, vp, sz, vp, vp, vp, sz, vp]),
            "nvcomp_zstd_batched_decompress_get_temp_size_v5": (sz, [sz, sz]),
            "nvcomp_zstd_batched_decompress_async_v5": (i, [vp, vp, vp, vp, sz, sz, vp, vp, vp, vp, sz, vp]),
            "nvcomp_zstd_batched_get_decompress_size_async_v5": (i, [vp, vp, vp, vp, vp, sz, vp]),
            "cuda_zstd_get_decompressed_sizes_async": (i, [vp, vp, vp, sz, vp, vp, vp]),
            "cuda_zstd_write_metadata_frame": (i, [vp, sz, i, psz, vp]),
            "cuda_zstd_stream_create": (vp, [i]),
            "cuda_zstd_stream_destroy": (None, [vp]),
            "cuda_zstd_stream_compress_chunk": (i, [vp, vp, sz, vp, psz, i, i, vp]),
            "cuda_zstd_stream_decompress_chunk": (i, [vp, vp, sz, vp, psz, pi, vp]),
            "cuda_zstd_stream_reset": (i, [vp]),
            "cuda_zstd_hybrid_create": (vp, [vp]),
            "cuda_zstd_hybrid_create_default": (vp, []),
            "cuda_zstd_hybrid_destroy": (None, [vp]),
            "cuda_zstd_hybrid_compress": (i, [vp, vp, sz, vp, psz, ctypes.c_uint, ctypes.c_uint, vp, vp]),
            "cuda_zstd_hybrid_decompress": (i, [vp, vp, sz, vp, psz, ctypes.c_uint, ctypes.c_uint, vp, vp]),
            "cuda_zstd_hybrid_max_compressed_size": (sz, [vp, sz]),
            "cuda_zstd_hybrid_query_routing": (ctypes.c_uint, [vp, sz, ctypes.c_uint, ctypes.c_uint, i]),
            "cuda_zstd_extract_metadata": (i, [vp, sz, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_uint), pi]),
            "cuda_zstd_hip_version": (ctypes.c_char_p, []),
            "cuda_zstd_hip_profile_enable": (None, [i]),
            "cuda_zstd_hip_profile_collect": (i, [ctypes.POINTER(ctypes.c_double)]),
            "cuda_zstd_hip_kernel_lds_bytes": (ctypes.c_uint, [i]),
            "cuda_zstd_seekable_max_size": (sz, [sz, sz, i]),
            "cuda_zstd_seekable_pack_get_temp_size": (sz, [sz]),
            "cuda_zstd_seekable_pack_async": (i, [vp, vp, vp, vp, vp, sz, sz, i, vp, sz, vp, vp, vp, sz, vp]),
            "cuda_zstd_seekable_info": (i, [vp, sz, psz, ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_uint), pi]),
            "cuda_zstd_seekable_read_get_temp_size": (sz, [sz, sz]),
            "cuda_zstd_seekable_read_get_temp_size_jobs": (sz, [sz, sz, sz]),
            "cuda_zstd_seekable_read": (i, [vp, vp, sz, ctypes.c_ulonglong, sz, vp, psz, i, vp, sz, vp]),
            "cuda_zstd_seekable_read_ranges_get_temp_size": (sz, [sz, sz, sz, sz]),
            "cuda_zstd_seekable_read_ranges": (i, [vp, vp, sz, vp, vp, vp, sz, sz, i, vp, psz, vp, sz, vp]),
            "cuda_zstd_seekable_index_get_temp_size": (sz, [sz, sz]),
            "cuda_zstd_seekable_index": (i, [vp, vp, sz, sz, vp, sz, psz, psz, ctypes.POINTER(ctypes.c_ulonglong), vp, sz, vp]),
            "cuda_zstd_hip_frames_index_path": (None, [i]),
            "cuda_zstd_hip_frames_index_last_path": (i, []),
            "cuda_zstd_hip_frames_index_split": (None, [i, ctypes.POINTER(ctypes.c_float)]),
            "cuda_zstd_set_long_distance": (i, [vp, i, ctypes.c_uint, ctypes.c_uint]),
            "cuda_zstd_set_checksum": (i, [vp, i]),
            "cuda_zstd_set_dict_entropy": (i, [vp, i]),
            "nvcomp_zstd_batch_set_dict_entropy_v5": (i, [vp, i]),
            "cuda_zstd_hip_ldm_plan": (ctypes.c_longlong, [vp, vp, sz, vp, sz, vp, sz, vp]),
            "cuda_zstd_hip_ldm_profile": (None, [i, ctypes.POINTER(ctypes.c_double)]),
            "cuda_zstd_hip_window_profile": (None, [i, ctypes.POINTER(ctypes.c_double)]),
            "cuda_zstd_adaptive_get_temp_size": (sz, [sz]),
            "cuda_zstd_adaptive_analyze_batch_async": (i, [vp, vp, sz, sz, i, vp, vp, vp, sz, vp]),
            "cuda_zstd_adaptive_select_level": (i, [vp, sz, sz, i, vp, vp]),
            "cuda_zstd_adaptive_finalize_host": (i, [ctypes.POINTER(ctypes.c_uint), ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, i, vp]),
        }
        for name, (res, args) in sig.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def error_string(code: int) -> str:
    return lib().cuda_zstd_get_error_string(code).decode()


def _test_fse_table(count, par):
    """Test hook (tests/test_gpu_tables.py): K2's FSE table builders alone, one wave per case.
    count: uint32 (n, 64); par: uint32 (n, 4) rows of maxSV, total, tableLog, useLowProbCount.
    Returns numpy arrays (norm per lane (n, 64), norm as stored (n, 64), NCount bytes (n, 256),
    NCount sizes (n), states (n, 512), symbol transforms (n, 64, 2) of dNb, dFS); what a case does
    not write keeps the fill byte 0xA5."""
    import numpy as np

    count, par = np.ascontiguousarray(count, np.uint32), np.ascontiguousarray(par, np.uint32)
    n = len(par)
    assert count.shape == (n, 64) and par.shape == (n, 4)
    out = [np.zeros((n, 64), np.int32), np.zeros((n, 64), np.int16), np.zeros((n, 256), np.uint8), np.zeros(n, np.uint32),
           np.zeros((n, 512), np.uint16), np.zeros((n, 64, 2), np.uint32)]
    f = lib().zh_test_fse_table
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p] * 2 + [ctypes.c_uint32] + [ctypes.c_void_p] * 6
    rc = f(count.ctypes.data, par.ctypes.data, n, *[a.ctypes.data for a in out])
    if rc:
        raise RuntimeError(f"zh_test_fse_table returned {rc}")
    return out


def _test_huf_table(count, par):
    """Test hook: K2's Huffman table builders alone, one wave per case.  count: uint32 (n, 256);
    par: uint32 (n, 2) rows of maxSV, maxNbBits.  Returns numpy arrays (huffLog (n), code lengths
    (n, 256), code values (n, 256), header bytes (n, 256), header sizes (n))."""
    import numpy as np

    count, par = np.ascontiguousarray(count, np.uint32), np.ascontiguousarray(par, np.uint32)
    n = len(par)
    assert count.shape == (n, 256) and par.shape == (n, 2)
    out = [np.zeros(n, np.uint32), np.zeros((n, 256), np.uint8), np.zeros((n, 256), np.uint16), np.zeros((n, 256), np.uint8),
           np.zeros(n, np.uint32)]
    f = lib().zh_test_huf_table
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p] * 2 + [ctypes.c_uint32] + [ctypes.c_void_p] * 5
    rc = f(count.ctypes.data, par.ctypes.data, n, *[a.ctypes.data for a in out])
    if rc:
        raise RuntimeError(f"zh_test_huf_table returned {rc}")
    return out


def _torch():
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("cuda_zstd: no GPU visible (the gfx950 path has no CPU fallback)")
    return torch


def _stream_ptr(stream) -> int:
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream


def max_compressed_size(n: int) -> int:
    """reference estimate_compressed_size (src/cuda_zstd_types.cpp:831-853)."""
    nb = max(1, (n + 128 * 1024 - 1) // (128 * 1024))
    return n + n // 255 + nb * 3 + 512


MIN_LEVEL, MAX_LEVEL, DEFAULT_LEVEL = 1, 22, 3
__version__ = "0.2.0"


def _is_host(x) -> bool:
    return isinstance(x, (bytes, bytearray, memoryview)) or type(x).__module__.startswith("numpy")


def _is_cuda_tensor(x) -> bool:
    return type(x).__module__ == "torch" and bool(getattr(x, "is_cuda", False))


def _to_device(x):
    """Host bytes-like / numpy -> uint8 device tensor (the reference binding's H2D)."""
    torch = _torch()
    import numpy as np

    a = np.frombuffer(bytes(x), np.uint8) if isinstance(x, (bytes, bytearray, memoryview)) else np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    if a.size == 0:
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.copy()).cuda()


def _host_bytes(t) -> bytes:
    return t.cpu().numpy().tobytes() if t.numel() else b""


def _frame_size(frame) -> int:
    """Content size from the frame header (after any skippable frames), like the reference's
    get_decompressed_size path of PyManager.decompress; 16x the input when it is absent."""
    try:
        return extract_metadata(frame)["uncompressed_size"] or frame.numel() * 16
    except ZstdError:
        return max(frame.numel() * 16, 1024)


class Manager:
    """C-ABI manager handle (reference PyManager, python/src/binding.cpp:151-329).

    Device tensors in -> device tensors out; host bytes / numpy in -> bytes out."""

    def __init__(self, level: int = 3, long_distance=False, hash_log: int = 0, checksum: bool = False, dict_entropy: bool = False):
        """long_distance: True = long-distance matching with a 2^27 window (`zstd --long`), an int =
        that window log (16..31); it applies to compress() of one buffer over 64 KiB.
        dict_entropy: with a formatted dictionary set, the first block of every frame starts from
        the dictionary's repcodes and may reuse its Huffman / FSE tables (treeless literals,
        Repeat_Mode); off, frames are what they were."""
        self.level = level
        self._h = lib().cuda_zstd_create_manager(level)
        if not self._h:
            raise ZstdError(INVALID, "cuda_zstd_create_manager")
        self._ws = None
        if long_distance:  # (False, None and 0: off)
            rc = lib().cuda_zstd_set_long_distance(self._h, 1, 0 if long_distance is True else int(long_distance), hash_log)
            if rc:
                self.close()
                raise ZstdError(rc, "cuda_zstd_set_long_distance")
        if checksum:
            lib().cuda_zstd_set_checksum(self._h, 1)
        if dict_entropy:
            lib().cuda_zstd_set_dict_entropy(self._h, 1)

    def close(self):
        if self._h:
            lib().cuda_zstd_destroy_manager(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may already be gone
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __repr__(self):
        return f"<cuda_zstd.Manager level={self.level}>"

    def get_level(self) -> int:
        return self.level

    def _workspace(self, nbytes: int):
        torch = _torch()
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device="cuda")
        return self._ws

    def compress(self, data, stream=None):
        """Compress a contiguous uint8 device tensor into one zstd frame (device tensor); host
        bytes-like / numpy input gives bytes (reference PyManager.compress)."""
        if _is_host(data):
            return _host_bytes(self.compress(_to_device(data), stream))
        torch = _torch()
        data = data.contiguous().view(torch.uint8)
        n = data.numel()
        out = torch.empty(max_compressed_size(n), dtype=torch.uint8, device=data.device)
        ws_n = lib().cuda_zstd_get_compress_workspace_size(self._h, n)
        ws = self._workspace(ws_n)
        size = ctypes.c_size_t(out.numel())
        rc = lib().cuda_zstd_compress(self._h, data.data_ptr(), n, out.data_ptr(), ctypes.byref(size), ws.data_ptr(), ws.numel(), _stream_ptr(stream))
        if rc:
            raise ZstdError(rc, "cuda_zstd_compress")
        return out[: size.value]

    def workspace_size(self, n: int) -> int:
        """Workspace bytes compress() of n bytes needs."""
        return lib().cuda_zstd_get_compress_workspace_size(self._h, n)

    def ldm_plan(self, data, stream=None):
        """The long-distance finder's decision for compress(data): a numpy uint32 array [cells, 3] of
        (seg_start, seg_len, distance) per 32 KiB cell, seg_len 0 = not split; no rows when
        long-distance matching does not apply."""
        import numpy as np

        torch = _torch()
        data = (_to_device(data) if _is_host(data) else data).contiguous().view(torch.uint8)
        n = data.numel()
        cells = (n + 32767) // 32768
        rec = np.zeros((max(cells, 1), 3), dtype=np.uint32)
        ws = self._workspace(self.workspace_size(n))
        got = lib().cuda_zstd_hip_ldm_plan(self._h, data.data_ptr(), n, rec.ctypes.data, cells, ws.data_ptr(), ws.numel(), _stream_ptr(stream))
        if got < 0:
            raise ZstdError(INVALID, "cuda_zstd_hip_ldm_plan")
        return rec[:got]

    @staticmethod
    def _batch_arrays(ins, caps):
        """compress_batch / decompress_batch: one output buffer with a 256-byte aligned slot of caps[k]
        bytes per item (its offsets), and the C arrays of the batch entries."""
        n = len(ins)
        offs = [0]
        for c in caps:
            offs.append(offs[-1] + ((max(c, 1) + 255) // 256) * 256)
        out = _torch().empty(max(offs[-1], 256), dtype=_torch().uint8, device="cuda")
        return (offs, out, (ctypes.c_void_p * n)(*[t.data_ptr() for t in ins]), (ctypes.c_void_p * n)(*[out.data_ptr() + o for o in offs[:-1]]),
                (ctypes.c_size_t * n)(*[t.numel() for t in ins]), (ctypes.c_size_t * n)(*caps), (ctypes.c_int * n)())

    def compress_batch(self, chunks: Sequence, stream=None) -> List:
        """ZstdBatchManager::compress_batch over a list of uint8 device tensors (host inputs:
        a list of bytes back)."""
        if len(chunks) and all(_is_host(c) for c in chunks):
            return [_host_bytes(o) for o in self.compress_batch([_to_device(c) for c in chunks], stream)]
        torch = _torch()
        n = len(chunks)
        ins = [c.contiguous().view(torch.uint8) for c in chunks]
        offs, out, in_ptrs, out_ptrs, in_sz, out_sz, st = self._batch_arrays(ins, [max_compressed_size(t.numel()) for t in ins])
        ws_n = lib().cuda_zstd_get_batch_compress_workspace_size(self._h, in_sz, n)
        ws = self._workspace(ws_n)
        rc = lib().cuda_zstd_compress_batch(self._h, in_ptrs, in_sz, n, out_ptrs, out_sz, st, ws.data_ptr(), ws.numel(), _stream_ptr(stream))
        if rc and all(s == OK for s in st):
            raise ZstdError(rc, "cuda_zstd_compress_batch")
        res = []
        for k in range(n):
            if st[k] != OK:
                raise ZstdError(st[k], f"cuda_zstd_compress_batch item {k}")
            res.append(out[offs[k] : offs[k] + out_sz[k]])
        return res

    def set_dictionary(self, d: "Dictionary"):
        """ZstdManager::set_dictionary: later compress / decompress calls use `d`."""
        rc = lib().cuda_zstd_set_dictionary(self._h, d._h)
        if rc:
            raise ZstdError(rc, "cuda_zstd_set_dictionary")

    def clear_dictionary(self):
        rc = lib().cuda_zstd_clear_dictionary(self._h)
        if rc:
            raise ZstdError(rc, "cuda_zstd_clear_dictionary")

    def decompress(self, frame, capacity: int = None, stream=None):
        """GPU-decode one device buffer (frames, concatenated) into a new device tensor of
        at most `capacity` bytes (cuda_zstd_decompress); capacity None: the exact size from
        decompressed_sizes (frames without a content size and concatenated frames included).
        Host bytes in -> bytes out (reference PyManager.decompress)."""
        if _is_host(frame):
            return _host_bytes(self.decompress(_to_device(frame), capacity, stream))
        torch = _torch()
        frame = frame.contiguous().view(torch.uint8)
        guess = False
        if capacity is None:
            capacity, guess = self._capacities([frame], stream)[0]
        # a guessed capacity (the size query rejected the buffer: the first frame's content size, or
        # 16x the input without one) grows on BUFFER_TOO_SMALL, and the decoder reports the error
        for _ in range(4 if guess else 1):
            out = torch.empty(max(capacity, 1), dtype=torch.uint8, device=frame.device)
            ws = self._workspace(lib().cuda_zstd_get_decompress_workspace_size(self._h, frame.numel()))
            size = ctypes.c_size_t(capacity)
            rc = lib().cuda_zstd_decompress(self._h, frame.data_ptr(), frame.numel(), out.data_ptr(), ctypes.byref(size), ws.data_ptr(),
                                            ws.numel(), _stream_ptr(stream))
            if rc == TOO_SMALL and guess:
                capacity *= 4
                continue
            if rc:
                raise ZstdError(rc, "cuda_zstd_decompress")
            return out[: size.value]
        raise ZstdError(TOO_SMALL, "cuda_zstd_decompress")

    def decompress_batch(self, frames: Sequence, capacities: Sequence[int] = None, stream=None, raise_on_error=True):
        """ZstdBatchManager::decompress_batch over device tensors: one GPU launch for all.
        Returns the decoded tensors (and, with raise_on_error=False, the nvcomp codes).
        capacities None: the exact sizes from one decompressed_sizes launch for the batch (a buffer
        that query rejects gets a guessed capacity, and the decoder's status for it is reported);
        host inputs give bytes back."""
        if len(frames) and all(_is_host(f) for f in frames):
            outs = self.decompress_batch([_to_device(f) for f in frames], capacities, stream, raise_on_error)
            if raise_on_error:
                return [_host_bytes(o) for o in outs]
            return [_host_bytes(o) for o in outs[0]], outs[1]
        torch = _torch()
        n = len(frames)
        ins = [f.contiguous().view(torch.uint8) for f in frames]
        if capacities is None:
            capacities = [c for c, _ in self._capacities(ins, stream)]
        offs, out, in_ptrs, out_ptrs, in_sz, out_sz, st = self._batch_arrays(ins, capacities)
        ws = self._workspace(lib().cuda_zstd_get_batch_decompress_workspace_size(self._h, in_sz, n))
        rc = lib().cuda_zstd_decompress_batch(self._h, in_ptrs, in_sz, n, out_ptrs, out_sz, st, ws.data_ptr(), ws.numel(), _stream_ptr(stream))
        if rc and all(s == OK for s in st):
            raise ZstdError(rc, "cuda_zstd_decompress_batch")
        res = [out[offs[k] : offs[k] + out_sz[k]] for k in range(n)]
        if raise_on_error:
            for k in range(n):
                if st[k] != OK:
                    raise ZstdError(st[k], f"cuda_zstd_decompress_batch item {k}")
            return res
        return res, list(st)

    def decompressed_sizes(self, frames: Sequence, stream=None, raise_on_error=True):
        """The decompressed size of every buffer (frames, concatenated), computed on the device
        (cuda_zstd_get_decompressed_sizes_async): one launch and one copy back for the whole batch.
        Exact whether or not a frame states its content size -- frames of streaming writers do not.
        Returns a list of ints (and, with raise_on_error=False, the status values: 0, or what a
        decode of that buffer reports, its size then 0).  Host inputs are uploaded first."""
        torch = _torch()
        n = len(frames)
        if n == 0:
            return [] if raise_on_error else ([], [])
        ins = [(_to_device(f) if _is_host(f) else f).contiguous().view(torch.uint8) for f in frames]
        s = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(s):
            args = torch.tensor([t.data_ptr() for t in ins] + [t.numel() for t in ins], dtype=torch.int64).cuda()
            res = torch.empty(2 * n, dtype=torch.int64, device="cuda")  # n sizes, then n int32 statuses
            rc = lib().cuda_zstd_get_decompressed_sizes_async(self._h, args.data_ptr(), args.data_ptr() + 8 * n, n, res.data_ptr(),
                                                              res.data_ptr() + 8 * n, s.cuda_stream)
            if rc:
                raise ZstdError(rc, "cuda_zstd_get_decompressed_sizes_async")
            host = res.cpu()
        sizes = [v & 0xFFFFFFFFFFFFFFFF for v in host[:n].tolist()]
        st = host[n:].view(torch.int32)[:n].tolist()
        if raise_on_error:
            for k in range(n):
                if st[k] != OK:
                    raise ZstdError(st[k], f"cuda_zstd_get_decompressed_sizes_async item {k}")
            return sizes
        return sizes, st

    def _capacities(self, ins, stream):
        """(capacity, guessed) per device buffer for a decode without given capacities: the exact
        size from one decompressed_sizes launch; where that rejects a buffer, _frame_size's guess, so
        that the decoder is the one to report the buffer's error."""
        sizes, st = self.decompressed_sizes(ins, stream, raise_on_error=False)
        return [(max(sz, 1), False) if c == OK else (_frame_size(f), True) for f, sz, c in zip(ins, sizes, st)]


class Dictionary:
    """Dictionary handle (reference dictionary::Dictionary, include/cuda_zstd_dictionary.h:101;
    DictionaryTrainer::train_dictionary, DictionaryManager::load_dictionary :292).  Raw content,
    or a formatted RFC 8878 §5 dictionary such as ZDICT_trainFromBuffer's."""

    def __init__(self, handle, what: str = "dictionary"):
        if not handle:
            raise ZstdError(INVALID, what)
        self._h = handle

    @classmethod
    def train(cls, samples, dict_size: int, k: int = 0, d: int = 0, stream=None, finalize: bool = False, level: int = 3) -> "Dictionary":
        """COVER training -> raw content; k = segment bytes, d = d-mer bytes (0: 1024 / 8).
        finalize=True: the trained content goes through finalize(samples, level), so the result is
        a formatted dictionary (dict_size bytes of content plus its entropy section).
        Host samples (bytes-like / uint8 arrays) train on the host.  Torch CUDA tensors -- a list
        or tuple of them, or one 2-D uint8 tensor with a sample per row -- train on the device
        (cuda_zstd_train_dictionary_device), ordered on `stream`; the bytes are the same."""
        if finalize:
            return cls.train(samples, dict_size, k, d, stream).finalize(samples, level, stream=stream)
        if _is_cuda_tensor(samples) or (isinstance(samples, (list, tuple)) and len(samples) and all(_is_cuda_tensor(t) for t in samples)):
            return cls._train_device(samples, dict_size, k, d, stream)
        raw = [bytes(s) for s in samples]
        bufs = [ctypes.create_string_buffer(b, max(len(b), 1)) for b in raw]
        n = len(raw)
        ptrs = (ctypes.c_void_p * n)(*[ctypes.addressof(b) for b in bufs])
        sizes = (ctypes.c_size_t * n)(*[len(b) for b in raw])
        if k or d:
            return cls(lib().cuda_zstd_train_dictionary_params(ptrs, sizes, n, dict_size, k, d), "cuda_zstd_train_dictionary_params")
        return cls(lib().cuda_zstd_train_dictionary(ptrs, sizes, n, dict_size), "cuda_zstd_train_dictionary")

    @classmethod
    def _train_device(cls, samples, dict_size, k, d, stream):
        torch = _torch()
        s = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(s):  # the concatenation and the temp buffer are ordered on the same stream
            if _is_cuda_tensor(samples):
                if samples.dim() != 2 or samples.dtype != torch.uint8:
                    raise TypeError("Dictionary.train: a single tensor must be 2-D uint8, one sample per row")
                sizes = [samples.shape[1]] * samples.shape[0]
                flat = samples.contiguous().view(-1)
            else:
                views = [t.contiguous().view(torch.uint8).view(-1) for t in samples]
                sizes = [v.numel() for v in views]
                flat = torch.cat(views) if len(views) > 1 else views[0]
            n = len(sizes)
            csz = (ctypes.c_size_t * max(n, 1))(*sizes)
            temp = torch.empty(max(lib().cuda_zstd_train_dictionary_device_get_temp_size(flat.numel(), n, dict_size, k), 256),
                               dtype=torch.uint8, device=flat.device)
            h = ctypes.c_void_p()
            rc = lib().cuda_zstd_train_dictionary_device(flat.data_ptr(), csz, n, dict_size, k, d, temp.data_ptr(), temp.numel(),
                                                         s.cuda_stream, ctypes.byref(h))
        if rc:
            raise ZstdError(rc, "cuda_zstd_train_dictionary_device")
        return cls(h.value, "cuda_zstd_train_dictionary_device")

    @classmethod
    def train_groups(cls, groups, dict_size: int, k: int = 0, d: int = 0, stream=None) -> List[Optional["Dictionary"]]:
        """One COVER dictionary (raw content) per group of samples, all trained on the device in one
        call (cuda_zstd_train_dictionaries_device): up to 4,096 groups, 64 of them in flight at a
        time.  Each group is a list or tuple of torch CUDA tensors, or one 2-D uint8 CUDA tensor
        with a sample per row (the forms train takes on the device); a group may be empty.  The
        concatenation and the temp buffer are ordered on `stream`.  Entry g equals
        Dictionary.train on group g's samples alone; it is None where the group gave fewer than
        256 bytes (status 12).  dict_size, k and d are common to the call, and all samples
        together stay under 2^32 - 64 bytes: train more data in a second call.
        Not done here: finalizing the contents (Dictionary.finalize per dictionary), host samples,
        per-group dict_size / k / d, and keeping the trained bytes on the device."""
        torch = _torch()
        s = stream if stream is not None else torch.cuda.current_stream()
        groups = list(groups)
        ng = len(groups)
        with torch.cuda.stream(s):  # the concatenation and the temp buffer are ordered on the same stream
            views, sizes, counts = [], [], []
            for grp in groups:
                if _is_cuda_tensor(grp):
                    if grp.dim() != 2 or grp.dtype != torch.uint8:
                        raise TypeError("Dictionary.train_groups: a group given as one tensor must be 2-D uint8, one sample per row")
                    views.append(grp.contiguous().view(-1))
                    sizes += [grp.shape[1]] * grp.shape[0]
                    counts.append(grp.shape[0])
                elif isinstance(grp, (list, tuple)) and all(_is_cuda_tensor(t) for t in grp):
                    rows = [t.contiguous().view(torch.uint8).view(-1) for t in grp]
                    views += rows
                    sizes += [v.numel() for v in rows]
                    counts.append(len(rows))
                else:
                    raise TypeError("Dictionary.train_groups: a group is a list or tuple of CUDA tensors, or one 2-D uint8 CUDA tensor")
            n = len(sizes)
            if n == 0:
                raise ZstdError(INVALID, "Dictionary.train_groups: no samples")
            flat = torch.cat(views) if len(views) > 1 else views[0]
            csz = (ctypes.c_size_t * n)(*sizes)
            ccn = (ctypes.c_size_t * max(ng, 1))(*counts)
            need = lib().cuda_zstd_train_dictionaries_device_get_temp_size(csz, n, ccn, ng, dict_size, k)
            temp = torch.empty(max(need, 256), dtype=torch.uint8, device=flat.device)
            hs = (ctypes.c_void_p * max(ng, 1))()
            st = (ctypes.c_int * max(ng, 1))()
            rc = lib().cuda_zstd_train_dictionaries_device(flat.data_ptr(), csz, n, ccn, ng, dict_size, k, d, temp.data_ptr(), temp.numel(),
                                                           s.cuda_stream, hs, st)
        if rc:
            raise ZstdError(rc, "cuda_zstd_train_dictionaries_device")
        return [cls(hs[g], "cuda_zstd_train_dictionaries_device") if hs[g] else None for g in range(ng)]

    def finalize(self, samples, level: int = 3, dict_id: int = 0, stream=None) -> "Dictionary":
        """This dictionary's content plus entropy tables -> a formatted RFC 8878 dictionary
        (libzstd's ZDICT_finalizeDictionary; cuda_zstd_finalize_dictionary).  The tables come from
        compressing the samples against the content at `level` on the device: host samples
        (bytes-like / uint8 arrays) are uploaded, torch CUDA tensors (a list, or one 2-D uint8
        tensor with a sample per row) are read in place.  dict_id 0: libzstd's hash rule.  Use the
        result with Manager(..., dict_entropy=True)."""
        keep = []
        if _is_cuda_tensor(samples):
            torch = _torch()
            if samples.dim() != 2 or samples.dtype != torch.uint8:
                raise TypeError("Dictionary.finalize: a single tensor must be 2-D uint8, one sample per row")
            samples = list(samples.contiguous())
        ptrs, sizes = [], []
        for s in samples:
            if _is_cuda_tensor(s):
                t = s.contiguous().view(_torch().uint8).view(-1)
                keep.append(t)
                ptrs.append(t.data_ptr())
                sizes.append(t.numel())
            else:
                b = bytes(s)
                cb = ctypes.create_string_buffer(b, max(len(b), 1))
                keep.append(cb)
                ptrs.append(ctypes.addressof(cb))
                sizes.append(len(b))
        n = len(ptrs)
        h = ctypes.c_void_p()
        if keep and any(_is_cuda_tensor(t) for t in keep):
            _torch().cuda.synchronize()  # the samples' producers have finished
        rc = lib().cuda_zstd_finalize_dictionary(self._h, (ctypes.c_void_p * max(n, 1))(*ptrs), (ctypes.c_size_t * max(n, 1))(*sizes), n, level,
                                                 dict_id, _stream_ptr(stream), ctypes.byref(h))
        if rc:
            raise ZstdError(rc, "cuda_zstd_finalize_dictionary")
        return Dictionary(h.value, "cuda_zstd_finalize_dictionary")

    @classmethod
    def load(cls, buf) -> "Dictionary":
        b = bytes(buf)
        cb = ctypes.create_string_buffer(b, max(len(b), 1))
        return cls(lib().cuda_zstd_load_dictionary(cb, len(b)), "cuda_zstd_load_dictionary")

    def content(self) -> bytes:
        n = lib().cuda_zstd_get_dictionary_content(self._h, None, 0)
        cb = ctypes.create_string_buffer(max(n, 1))
        lib().cuda_zstd_get_dictionary_content(self._h, cb, n)
        return cb.raw[:n]

    def layout(self):
        """(Dictionary_ID, content offset); (0, 0) for raw content."""
        did, off = ctypes.c_uint(), ctypes.c_size_t()
        rc = lib().cuda_zstd_get_dictionary_layout(self._h, ctypes.byref(did), ctypes.byref(off))
        if rc:
            raise ZstdError(rc, "cuda_zstd_get_dictionary_layout")
        return did.value, off.value

    def close(self):
        if self._h:
            lib().cuda_zstd_destroy_dictionary(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass


class DictionarySet:
    """A set of dictionaries on the device (cuda_zstd_dict_set_create): 1 .. 4,096 Dictionary
    handles, raw content or formatted, for batches whose chunks use different dictionaries.  The
    bytes are copied (the handles may be closed afterwards) and the set is immutable.  Two
    dictionaries with the same non-zero Dictionary_ID raise; raw-content entries (ID 0) are
    reachable by index only.  Bind it with BatchedCompressor / BatchedDecompressor
    .set_dictionary_set, or use compress_batch_dicts / decompress_batch_dicts."""

    def __init__(self, dictionaries: Sequence["Dictionary"], stream=None):
        ds = list(dictionaries)
        n = len(ds)
        self._h = None
        h = ctypes.c_void_p()
        rc = lib().cuda_zstd_dict_set_create((ctypes.c_void_p * max(n, 1))(*[d._h for d in ds]), n, _stream_ptr(stream), ctypes.byref(h))
        if rc:
            raise ZstdError(rc, "cuda_zstd_dict_set_create")
        self._h = h.value

    @classmethod
    def train(cls, groups, dict_size: int, k: int = 0, d: int = 0, stream=None) -> "DictionarySet":
        """Dictionary.train_groups(groups, ...) straight into a set: entry g is the raw-content
        dictionary trained on group g's device samples.  Raises ZstdError(12) naming the first
        group that gave fewer than 256 bytes.  The same limits hold (common dict_size / k / d,
        under 2^32 - 64 sample bytes per call, device samples only), and the contents are not
        finalized: for formatted entries, finalize the dictionaries of train_groups one by one
        and build the set from them."""
        ds = Dictionary.train_groups(groups, dict_size, k, d, stream)
        for g, one in enumerate(ds):
            if one is None:
                raise ZstdError(12, f"DictionarySet.train: group {g} gave no dictionary")
        return cls(ds, stream)

    def __len__(self) -> int:
        return lib().cuda_zstd_dict_set_count(self._h)

    def find(self, dict_id: int) -> int:
        """Entry index of a non-zero Dictionary_ID, or -1."""
        return lib().cuda_zstd_dict_set_find(self._h, dict_id)

    def close(self):
        """Waits for the stream-ordered calls that read the set, then frees it (a handle it is still
        bound to keeps the device memory)."""
        if self._h:
            lib().cuda_zstd_dict_set_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass


class BatchedDecompressor:
    """Stream-ordered batched GPU decompression over device arrays
    (nvcomp_zstd_batched_decompress_async_v5).  Used by bench.py --decompress."""

    def __init__(self):
        self._h = lib().nvcomp_zstd_batch_create_v5(3, 64 * 1024, 0)
        if not self._h:
            raise ZstdError(INVALID, "nvcomp_zstd_batch_create_v5")

    def close(self):
        if self._h:
            lib().nvcomp_zstd_batch_destroy_v5(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def temp_size(num_chunks: int, max_out: int) -> int:
        return lib().nvcomp_zstd_batched_decompress_get_temp_size_v5(num_chunks, max_out)

    def decompress_async(self, d_in_ptrs, d_in_sizes, d_out_caps, max_out, d_out_ptrs, d_out_sizes, d_status, temp, stream=None):
        n = d_in_ptrs.numel()
        rc = lib().nvcomp_zstd_batched_decompress_async_v5(
            self._h, d_in_ptrs.data_ptr(), d_in_sizes.data_ptr(), d_out_caps.data_ptr() if d_out_caps is not None else None, max_out, n,
            d_out_ptrs.data_ptr(), d_out_sizes.data_ptr(), d_status.data_ptr() if d_status is not None else None, temp.data_ptr(), temp.numel(),
            _stream_ptr(stream))
        if rc:
            raise ZstdError(rc, "nvcomp_zstd_batched_decompress_async_v5")

    def decompress_prefix_async(self, d_in_ptrs, d_in_sizes, d_prefix_ptrs, d_prefix_sizes, d_out_caps, max_out, d_out_ptrs, d_out_sizes,
                                d_status, temp, stream=None):
        """decompress_async with one prefix per buffer (nvcomp_zstd_batched_decompress_prefix_async_v5):
        d_prefix_ptrs / d_prefix_sizes are int64 device tensors, size 0 = no prefix; the whole prefix
        is addressable in front of the frame.  Same workspace as decompress_async."""
        n = d_in_ptrs.numel()
        rc = lib().nvcomp_zstd_batched_decompress_prefix_async_v5(
            self._h, d_in_ptrs.data_ptr(), d_in_sizes.data_ptr(), d_prefix_ptrs.data_ptr() if d_prefix_ptrs is not None else None,
            d_prefix_sizes.data_ptr() if d_prefix_sizes is not None else None, d_out_caps.data_ptr() if d_out_caps is not None else None,
            max_out, n, d_out_ptrs.data_ptr(), d_out_sizes.data_ptr(), d_status.data_ptr() if d_status is not None else None,
            temp.data_ptr(), temp.numel(), _stream_ptr(stream))
        if rc:
            raise ZstdError(rc, "nvcomp_zstd_batched_decompress_prefix_async_v5")

    def set_dictionary(self, d: "Dictionary"):
        rc = lib().nvcomp_zstd_batch_set_dictionary_v5(self._h, d._h)
        if rc:
            raise ZstdError(rc, "nvcomp_zstd_batch_set_dictionary_v5")

    def set_dictionary_set(self, s: "DictionarySet"):
        """Bind a dictionary set (None clears): decompress_async and get_sizes_async then resolve every
        frame's dictionary from its Dictionary_ID on the device; decompress_dicts_async also takes
        entry indices.  Not together with set_dictionary."""
        rc = lib().nvcomp_zstd_batch_set_dictionary_set_v5(self._h, s._h if s is not None else None)
        if rc:
            raise ZstdError(rc, "nvcomp_zstd_batch_set_dictionary_set_v5")

    def decompress_dicts_async(self, d_in_ptrs, d_in_sizes, d_dict_index, d_out_caps, max_out, d_out_ptrs, d_out_sizes, d_status, temp,
                               stream=None):
        """decompress_async against the bound set (nvcomp_zstd_batched_decompress_dicts_async_v5):
        d_dict_index is an int32 device tensor or None; -1 (or None) resolves a frame by its
        Dictionary_ID, an index >= 0 names the entry (a raw-content entry's frames carry no ID).
        Same workspace as decompress_async."""
        n = d_in_ptrs.numel()
        rc = lib().nvcomp_zstd_batched_decompress_dicts_async_v5(
            self._h, d_in_ptrs.data_ptr(), d_in_sizes.data_ptr(), d_dict_index.data_ptr() if d_dict_index is not None else None,
            d_out_caps.data_ptr() if d_out_caps is not None else None, max_out, n, d_out_ptrs.data_ptr(), d_out_sizes.data_ptr(),
            d_status.data_ptr() if d_status is not None else None, temp.data_ptr(), temp.numel(), _stream_ptr(stream))
        if rc:
            raise ZstdError(rc, "nvcomp_zstd_batched_decompress_dicts_async_v5")

    def get_sizes_async(self, d_in_ptrs, d_in_sizes, d_out_sizes, d_status, stream=None):
        """The decompressed size of every buffer, on the device
        (nvcomp_zstd_batched_get_decompress_size_async_v5): int64 device tensors of pointers and
        sizes in, sizes (int64) and nvcomp codes (int32, or None) out; one launch, stream-ordered,
        no workspace.  Exact whether or not a frame states its content size."""
        n = d_in_ptrs.numel()
        rc = lib().nvcomp_zstd_batched_get_decompress_size_async_v5(
            self._h, d_in_ptrs.data_ptr(), d_in_sizes.data_ptr(), d_out_sizes.data_ptr(), d_status.data_ptr() if d_status is not None else None, n,
            _stream_ptr(stream))
        if rc:
            raise ZstdError(rc, "nvcomp_zstd_batched_get_decompress_size_async_v5")


class BatchedCompressor:
    """Stream-ordered batched compression of equal-capacity chunk slots
    (nvcomp_zstd_batched_compress_async_v5).  Used by bench.py."""

    def __init__(self, level: int = 3, chunk_size: int = 64 * 1024, checksum: bool = False, dict_entropy: bool = False):
        """dict_entropy: as Manager's (nvcomp_zstd_batch_set_dict_entropy_v5)."""
        self._h = lib().nvcomp_zstd_batch_create_v5(level, chunk_size, 1 if checksum else 0)
        if not self._h:
            raise ZstdError(INVALID, "nvcomp_zstd_batch_create_v5")
        self.chunk_size = chunk_size
        if dict_entropy:
            lib().nvcomp_zstd_batch_set_dict_entropy_v5(self._h, 1)

    def close(self):
        if self._h:
            lib().nvcomp_zstd_batch_destroy_v5(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def temp_size(self, num_chunks: int, max_chunk: int) -> int:
        """Workspace of compress_async for this handle's level and dictionary."""
        return lib().nvcomp_zstd_batch_get_batched_temp_size_v5(self._h, num_chunks, max_chunk)

    def temp_size_for(self, chunk_sizes) -> int:
        """Workspace for these chunk sizes under the handle's current dictionary."""
        n = len(chunk_sizes)
        arr = (ctypes.c_size_t * n)(*chunk_sizes)
        return lib().nvcomp_zstd_batch_get_compress_temp_size_v5(self._h, arr, n)

    def set_dictionary(self, d: "Dictionary"):
        rc = lib().nvcomp_zstd_batch_set_dictionary_v5(self._h, d._h)
        if rc:
            raise ZstdError(rc, "nvcomp_zstd_batch_set_dictionary_v5")

    def max_out(self, max_chunk: int) -> int:
        return lib().nvcomp_zstd_batch_get_max_compressed_chunk_size_v5(self._h, max_chunk)

    def compress_async(self, d_in_ptrs, d_in_sizes, max_chunk, d_out_ptrs, d_out_sizes, d_status, temp, stream=None):
        n = d_in_ptrs.numel()
        rc = lib().nvcomp_zstd_batched_compress_async_v5(
            self._h, d_in_ptrs.data_ptr(), d_in_sizes.data_ptr(), max_chunk, n, d_out_ptrs.data_ptr(), d_out_sizes.data_ptr(),
            d_status.data_ptr() if d_status is not None else None, temp.data_ptr(), temp.numel(), _stream_ptr(stream))
        if rc:
            raise ZstdError(rc, "nvcomp_zstd_batched_compress_async_v5")

    @staticmethod
    def temp_size_levels(num_chunks: int, max_chunk: int) -> int:
        """Workspace of compress_levels_async (nvcomp_zstd_batched_compress_levels_get_temp_size_v5)."""
        return lib().nvcomp_zstd_batched_compress_levels_get_temp_size_v5(num_chunks, max_chunk)

    def compress_levels_async(self, d_in_ptrs, d_in_sizes, d_levels, max_chunk, d_out_ptrs, d_out_sizes, d_status, temp, stream=None):
        """compress_async at one level per chunk: d_levels is a device int32 tensor (such as
        analyze_batch_device's), read on the device in stream order; the handle's level is not
        used, its checksum setting is (nvcomp_zstd_batched_compress_levels_async_v5).  No
        dictionary."""
        n = d_in_ptrs.numel()
        rc = lib().nvcomp_zstd_batched_compress_levels_async_v5(
            self._h, d_in_ptrs.data_ptr(), d_in_sizes.data_ptr(), d_levels.data_ptr() if d_levels is not None else None, max_chunk, n,
            d_out_ptrs.data_ptr(), d_out_sizes.data_ptr(), d_status.data_ptr() if d_status is not None else None, temp.data_ptr(),
            temp.numel(), _stream_ptr(stream))
        if rc:
            raise ZstdError(rc, "nvcomp_zstd_batched_compress_levels_async_v5")

    def temp_size_prefix(self, num_chunks: int, max_chunk: int) -> int:
        """Workspace of compress_prefix_async (nvcomp_zstd_batch_get_batched_prefix_temp_size_v5)."""
        return lib().nvcomp_zstd_batch_get_batched_prefix_temp_size_v5(self._h, num_chunks, max_chunk)

    def compress_prefix_async(self, d_in_ptrs, d_in_sizes, d_prefix_ptrs, d_prefix_sizes, max_chunk, d_out_ptrs, d_out_sizes, d_status, temp,
                              stream=None):
        """compress_async with one prefix per chunk (nvcomp_zstd_batched_compress_prefix_async_v5):
        d_prefix_ptrs / d_prefix_sizes are int64 device tensors; chunk i is compressed behind the
        bytes at d_prefix_ptrs[i] as a raw-content dictionary (size 0: a plain frame).  No handle
        dictionary, no per-chunk levels."""
        n = d_in_ptrs.numel()
        rc = lib().nvcomp_zstd_batched_compress_prefix_async_v5(
            self._h, d_in_ptrs.data_ptr(), d_in_sizes.data_ptr(), d_prefix_ptrs.data_ptr() if d_prefix_ptrs is not None else None,
            d_prefix_sizes.data_ptr() if d_prefix_sizes is not None else None, max_chunk, n, d_out_ptrs.data_ptr(), d_out_sizes.data_ptr(),
            d_status.data_ptr() if d_status is not None else None, temp.data_ptr(), temp.numel(), _stream_ptr(stream))
        if rc:
            raise ZstdError(rc, "nvcomp_zstd_batched_compress_prefix_async_v5")

    def set_dictionary_set(self, s: "DictionarySet"):
        """Bind a dictionary set for compress_dicts_async (None clears).  Not together with
        set_dictionary."""
        rc = lib().nvcomp_zstd_batch_set_dictionary_set_v5(self._h, s._h if s is not None else None)
        if rc:
            raise ZstdError(rc, "nvcomp_zstd_batch_set_dictionary_set_v5")

    def temp_size_dicts(self, num_chunks: int, max_chunk: int) -> int:
        """Workspace of compress_dicts_async (nvcomp_zstd_batch_get_batched_dicts_temp_size_v5)."""
        return lib().nvcomp_zstd_batch_get_batched_dicts_temp_size_v5(self._h, num_chunks, max_chunk)

    def compress_dicts_async(self, d_in_ptrs, d_in_sizes, d_dict_index, max_chunk, d_out_ptrs, d_out_sizes, d_status, temp, stream=None):
        """compress_async with one entry of the bound set per chunk
        (nvcomp_zstd_batched_compress_dicts_async_v5): d_dict_index is an int32 device tensor, read
        on the device; -1 = no dictionary.  Frame i is what a handle with that one dictionary set
        writes for chunk i."""
        n = d_in_ptrs.numel()
        rc = lib().nvcomp_zstd_batched_compress_dicts_async_v5(
            self._h, d_in_ptrs.data_ptr(), d_in_sizes.data_ptr(), d_dict_index.data_ptr() if d_dict_index is not None else None, max_chunk, n,
            d_out_ptrs.data_ptr(), d_out_sizes.data_ptr(), d_status.data_ptr() if d_status is not None else None, temp.data_ptr(),
            temp.numel(), _stream_ptr(stream))
        if rc:
            raise ZstdError(rc, "nvcomp_zstd_batched_compress_dicts_async_v5")

    @staticmethod
    def seekable_max_size(num_frames: int, max_compressed_chunk: int, checksums: bool = False) -> int:
        return lib().cuda_zstd_seekable_max_size(num_frames, max_compressed_chunk, 1 if checksums else 0)

    @staticmethod
    def pack_temp_size(num_frames: int) -> int:
        return lib().cuda_zstd_seekable_pack_get_temp_size(num_frames)

    def pack_seekable_async(self, d_frame_ptrs, d_frame_sizes, d_frame_status, d_in_ptrs, d_in_sizes, max_compressed_chunk, out, d_out_size,
                            d_status, temp, checksums: bool = False, stream=None):
        """Stream-ordered pack of compress_async's frames into one seekable stream in `out`
        (cuda_zstd_seekable_pack_async): the frames back to back, then the seek table.  Every
        argument is a device tensor; d_out_size (int64[1]) and d_status (int32[1]) receive the
        stream's size and an nvcomp-style code.  d_in_ptrs is only read with checksums."""
        n = d_frame_ptrs.numel()
        rc = lib().cuda_zstd_seekable_pack_async(
            d_frame_ptrs.data_ptr(), d_frame_sizes.data_ptr(), d_frame_status.data_ptr() if d_frame_status is not None else None,
            d_in_ptrs.data_ptr() if d_in_ptrs is not None else None, d_in_sizes.data_ptr(), n, max_compressed_chunk, 1 if checksums else 0,
            out.data_ptr(), out.numel(), d_out_size.data_ptr(), d_status.data_ptr(), temp.data_ptr(), temp.numel(), _stream_ptr(stream))
        if rc:
            raise ZstdError(rc, "cuda_zstd_seekable_pack_async")


BatchManager = BatchedCompressor  # the batch manager of the C ABI (nvcomp_zstd_batch_*_v5) under its other name


class StreamingManager:
    """ZstdStreamingManager over the C ABI (cuda_zstd_stream_*; reference
    include/cuda_zstd_manager.h:300-352).  Each chunk is a complete frame; with_history=True is
    compress_chunk_with_history (the preceding <= 64 KiB of the stream as history, reference
    src/cuda_zstd_manager.cu:6327-6418); decompress_chunk keeps the decoded window, so chunks
    must be decoded in stream order.  Device tensors."""

    def __init__(self, level: int = 3):
        self._h = lib().cuda_zstd_stream_create(level)
        if not self._h:
            raise ZstdError(INVALID, "cuda_zstd_stream_create")

    def close(self):
        if self._h:
            lib().cuda_zstd_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def compress_chunk(self, data, with_history: bool = True, is_last: bool = False, stream=None):
        torch = _torch()
        data = data.contiguous().view(torch.uint8)
        out = torch.empty(max_compressed_size(data.numel()), dtype=torch.uint8, device=data.device)
        size = ctypes.c_size_t(out.numel())
        rc = lib().cuda_zstd_stream_compress_chunk(self._h, data.data_ptr(), data.numel(), out.data_ptr(), ctypes.byref(size), int(with_history),
                                                   int(is_last), _stream_ptr(stream))
        if rc:
            raise ZstdError(rc, "cuda_zstd_stream_compress_chunk")
        return out[: size.value]

    def decompress_chunk(self, frame, capacity: int = None, stream=None):
        torch = _torch()
        frame = frame.contiguous().view(torch.uint8)
        auto = capacity is None
        if auto:
            capacity = _frame_size(frame)
        for _ in range(4 if auto else 1):  # (a derived capacity grows on BUFFER_TOO_SMALL)
            out = torch.empty(max(capacity, 1), dtype=torch.uint8, device=frame.device)
            size = ctypes.c_size_t(capacity)
            last = ctypes.c_int()
            rc = lib().cuda_zstd_stream_decompress_chunk(self._h, frame.data_ptr(), frame.numel(), out.data_ptr(), ctypes.byref(size),
                                                         ctypes.byref(last), _stream_ptr(stream))
            if rc == TOO_SMALL and auto:
                capacity *= 4
                continue
            if rc:
                raise ZstdError(rc, "cuda_zstd_stream_decompress_chunk")
            return out[: size.value]
        raise ZstdError(TOO_SMALL, "cuda_zstd_stream_decompress_chunk")

    def reset(self):
        rc = lib().cuda_zstd_stream_reset(self._h)
        if rc:
            raise ZstdError(rc, "cuda_zstd_stream_reset")


class StreamBatch:
    """Many streams in one call (cuda_zstd_stream_batch_*): num_streams streams whose 64 KiB
    windows stay on the device.  compress_chunks / decompress_chunks take one chunk per stream
    (uint8 device tensors; None or an empty tensor: the stream is idle this round) and return one
    tensor per stream (None for an idle or failed stream) plus the statuses.  Frame i is what a
    StreamingManager of stream i writes with history."""

    def __init__(self, level: int, num_streams: int, max_chunk: int):
        self._h = lib().cuda_zstd_stream_batch_create(level, num_streams, max_chunk)
        if not self._h:
            raise ZstdError(INVALID, "cuda_zstd_stream_batch_create")
        self.num_streams, self.max_chunk = num_streams, max_chunk
        self.max_out = lib().cuda_zstd_stream_batch_max_compressed_chunk_size(self._h)

    def close(self):
        if self._h:
            lib().cuda_zstd_stream_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def compress_async(self, d_in_ptrs, d_in_sizes, d_out_ptrs, d_out_sizes, d_status, stream=None):
        """The raw call over int64 device tensors (cuda_zstd_stream_batch_compress_async)."""
        rc = lib().cuda_zstd_stream_batch_compress_async(self._h, d_in_ptrs.data_ptr(), d_in_sizes.data_ptr(), d_out_ptrs.data_ptr(),
                                                         d_out_sizes.data_ptr(), d_status.data_ptr() if d_status is not None else None,
                                                         _stream_ptr(stream))
        if rc:
            raise ZstdError(rc, "cuda_zstd_stream_batch_compress_async")

    def decompress_async(self, d_in_ptrs, d_in_sizes, d_out_caps, d_out_ptrs, d_out_sizes, d_status, stream=None):
        rc = lib().cuda_zstd_stream_batch_decompress_async(self._h, d_in_ptrs.data_ptr(), d_in_sizes.data_ptr(),
                                                           d_out_caps.data_ptr() if d_out_caps is not None else None, d_out_ptrs.data_ptr(),
                                                           d_out_sizes.data_ptr(), d_status.data_ptr() if d_status is not None else None,
                                                           _stream_ptr(stream))
        if rc:
            raise ZstdError(rc, "cuda_zstd_stream_batch_decompress_async")

    def _round(self, items, slot, decode, stream):
        torch = _torch()
        n = self.num_streams
        if len(items) != n:
            raise ZstdError(INVALID, "StreamBatch: one chunk (or None) per stream")
        s = stream if stream is not None else torch.cuda.current_stream()
        ins = [None if c is None else c.contiguous().view(torch.uint8) for c in items]
        sizes = [0 if t is None else t.numel() for t in ins]
        with torch.cuda.stream(s):
            out = torch.empty(n * slot, dtype=torch.uint8, device="cuda")
            table = torch.tensor([[0 if t is None or not t.numel() else t.data_ptr() for t in ins], sizes,
                                  [out.data_ptr() + k * slot for k in range(n)]], dtype=torch.int64)
            d_table = table.pin_memory().to("cuda", non_blocking=True)
            if s != torch.cuda.current_stream():
                for t in ins:
                    if t is not None:
                        t.record_stream(s)
            d_sizes = torch.zeros(n, dtype=torch.int64, device="cuda")
            d_status = torch.zeros(n, dtype=torch.int32, device="cuda")
            if decode:
                self.decompress_async(d_table[0], d_table[1], None, d_table[2], d_sizes, d_status, s)
            else:
                self.compress_async(d_table[0], d_table[1], d_table[2], d_sizes, d_status, s)
            got_sizes, got_status = torch.stack([d_sizes, d_status.to(torch.int64)]).cpu().tolist()
        res = [out[k * slot : k * slot + got_sizes[k]] if got_status[k] == OK else None for k in range(n)]
        return res, got_status

    def compress_chunks(self, chunks: Sequence, stream=None):
        """-> (frames, statuses): frame i of stream i's chunk behind its window; every window advances."""
        return self._round(chunks, ((self.max_out + 255) // 256) * 256, False, stream)

    def decompress_chunks(self, frames: Sequence, stream=None):
        """-> (chunks, statuses): the frames of one round, decoded behind the decoded windows."""
        return self._round(frames, ((self.max_chunk + 255) // 256) * 256, True, stream)

    def reset(self, stream=None):
        rc = lib().cuda_zstd_stream_batch_reset(self._h, _stream_ptr(stream))
        if rc:
            raise ZstdError(rc, "cuda_zstd_stream_batch_reset")


# HybridEngine (reference PyHybridEngine, python/src/binding.cpp:331-545, over
# cuda_zstd_hybrid_*): host buffers in and out; the engine routes between libzstd on the host
# and the GPU (cuda_zstd_hybrid_query_routing tells which).
HOST, DEVICE, MANAGED, UNKNOWN = 0, 1, 2, 3  # DataLocation
AUTO, PREFER_CPU, PREFER_GPU, FORCE_CPU, FORCE_GPU, ADAPTIVE = range(6)  # HybridMode
CPU_LIBZSTD, GPU_KERNELS, CPU_PARALLEL = 0, 1, 2  # ExecutionBackend


class HybridConfig(ctypes.Structure):
    """cuda_zstd_hybrid_config_t (reference HybridConfig, include/cuda_zstd_hybrid.h:45-70)."""
    _fields_ = [("mode", ctypes.c_uint), ("cpu_size_threshold", ctypes.c_size_t), ("gpu_device_threshold", ctypes.c_size_t),
                ("compression_level", ctypes.c_int), ("enable_profiling", ctypes.c_int), ("cpu_thread_count", ctypes.c_uint)]


class HybridResult(ctypes.Structure):
    _fields_ = [("backend_used", ctypes.c_uint), ("input_location", ctypes.c_uint), ("output_location", ctypes.c_uint),
                ("total_time_ms", ctypes.c_double), ("transfer_time_ms", ctypes.c_double), ("compute_time_ms", ctypes.c_double),
                ("throughput_mbps", ctypes.c_double), ("input_bytes", ctypes.c_size_t), ("output_bytes", ctypes.c_size_t),
                ("compression_ratio", ctypes.c_float)]


class HybridEngine:
    def __init__(self, level_or_config=3):
        if isinstance(level_or_config, HybridConfig):
            self.config = level_or_config
        else:
            self.config = HybridConfig(AUTO, 1 << 20, 0, int(level_or_config), 0, 0)
        self._h = lib().cuda_zstd_hybrid_create(ctypes.byref(self.config))
        if not self._h:
            raise ZstdError(INVALID, "cuda_zstd_hybrid_create")
        self.last_result = None

    def close(self):
        if self._h:
            lib().cuda_zstd_hybrid_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __repr__(self):
        return f"<cuda_zstd.HybridEngine level={self.config.compression_level}>"

    def get_level(self) -> int:
        return self.config.compression_level

    def get_config(self) -> HybridConfig:
        return self.config

    def query_routing(self, size: int, input_loc: int = HOST, output_loc: int = HOST, is_compression: bool = True) -> int:
        return lib().cuda_zstd_hybrid_query_routing(self._h, size, input_loc, output_loc, int(is_compression))

    def compress(self, data) -> bytes:
        b = bytes(data)
        if not b:
            return b""
        src = ctypes.create_string_buffer(b, len(b))
        cap = lib().cuda_zstd_hybrid_max_compressed_size(self._h, len(b))
        dst = ctypes.create_string_buffer(cap)
        size, res = ctypes.c_size_t(cap), HybridResult()
        rc = lib().cuda_zstd_hybrid_compress(self._h, src, len(b), dst, ctypes.byref(size), HOST, HOST, ctypes.byref(res), None)
        if rc:
            raise ZstdError(rc, "hybrid compress")
        self.last_result = res
        return dst.raw[: size.value]

    def decompress(self, data) -> bytes:
        b = bytes(data)
        if not b:
            return b""
        try:
            cap = extract_metadata(b)["uncompressed_size"] or max(16 * len(b), 1024)
        except ZstdError:
            cap = max(16 * len(b), 1024)
        src = ctypes.create_string_buffer(b, len(b))
        for _ in range(3):  # grow on BUFFER_TOO_SMALL, as the reference binding does
            dst = ctypes.create_string_buffer(max(cap, 1))
            size, res = ctypes.c_size_t(cap), HybridResult()
            rc = lib().cuda_zstd_hybrid_decompress(self._h, src, len(b), dst, ctypes.byref(size), HOST, HOST, ctypes.byref(res), None)
            if rc == 0:
                self.last_result = res
                return dst.raw[: size.value]
            if rc != TOO_SMALL:
                raise ZstdError(rc, "hybrid decompress")
            cap *= 4
        raise ZstdError(TOO_SMALL, "hybrid decompress")


def compress(data, level: int = 3, stream=None, long_distance=False):
    return Manager(level, long_distance=long_distance).compress(data, stream)


def ldm_plan(data, window_log: int = 27, hash_log: int = 20, stream=None):
    """Manager.ldm_plan with long-distance matching at that window and table size."""
    return Manager(3, long_distance=window_log, hash_log=hash_log).ldm_plan(data, stream)


def compress_batch(chunks, level: int = 3, stream=None):
    return Manager(level).compress_batch(chunks, stream)


def decompress(frame, capacity: int = None, stream=None):
    return Manager(3).decompress(frame, capacity, stream)


def decompress_batch(frames, capacities=None, stream=None):
    return Manager(3).decompress_batch(frames, capacities, stream)


def decompressed_sizes(frames, stream=None, raise_on_error=True):
    return Manager(3).decompressed_sizes(frames, stream, raise_on_error)


def seekable_compress(data, frame_size: int = 65536, level: int = 3, checksums: bool = False, stream=None):
    """Compress `data` as a Zstandard seekable stream: independent frames of `frame_size` bytes
    of content, then the seek table.  compress_async and pack_seekable_async are enqueued on one
    stream with no synchronisation between them; the only wait is for the stream's size, to
    trim the returned device tensor.  Host bytes / numpy in -> bytes out."""
    if _is_host(data):
        return _host_bytes(seekable_compress(_to_device(data), frame_size, level, checksums, stream))
    torch = _torch()
    if frame_size <= 0:
        raise ZstdError(INVALID, "seekable_compress frame_size")
    data = data.contiguous().view(torch.uint8).reshape(-1)
    total = data.numel()
    n = (total + frame_size - 1) // frame_size
    dev = data.device
    comp = BatchedCompressor(level, frame_size)
    slot = (comp.max_out(frame_size) + 255) // 256 * 256
    cap = BatchedCompressor.seekable_max_size(n, slot, checksums)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    out_size = torch.zeros(1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        idx = torch.arange(n, dtype=torch.int64, device=dev)
        in_ptrs = data.data_ptr() + idx * frame_size
        in_sizes = torch.clamp(total - idx * frame_size, max=frame_size)
        slots = torch.empty(max(n * slot, 1), dtype=torch.uint8, device=dev)
        f_ptrs = slots.data_ptr() + idx * slot
        f_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
        f_status = torch.zeros(n, dtype=torch.int32, device=dev)
        temp = torch.empty(max(comp.temp_size(n, frame_size), BatchedCompressor.pack_temp_size(n), 256), dtype=torch.uint8, device=dev)
        if n:
            comp.compress_async(in_ptrs, in_sizes, frame_size, f_ptrs, f_sizes, f_status, temp, s)
        comp.pack_seekable_async(f_ptrs, f_sizes, f_status, in_ptrs, in_sizes, slot, out, out_size, status, temp, checksums, s)
        for t in (data, slots, temp, out):
            t.record_stream(s)
        res = torch.stack([out_size[0], status[0].to(torch.int64)]).cpu()  # waits for the stream
    if int(res[1]):
        raise ZstdError(int(res[1]), "seekable_compress")
    return out[: int(res[0])]


class SeekableReader:
    """Random access into a Zstandard seekable stream held in device memory (host bytes are
    uploaded once, and reads then give bytes back).  `manager`: a BatchedCompressor /
    BatchedDecompressor whose handle (and dictionary) decodes the frames."""

    def __init__(self, buf, manager=None):
        torch = _torch()
        self._host = _is_host(buf)
        self._buf = _to_device(buf) if self._host else buf.contiguous().view(torch.uint8).reshape(-1)
        self._mgr = manager if manager is not None else BatchedDecompressor()
        n, tot, mx, ck = ctypes.c_size_t(0), ctypes.c_ulonglong(0), ctypes.c_uint(0), ctypes.c_int(0)
        rc = lib().cuda_zstd_seekable_info(self._buf.data_ptr() if self._buf.numel() else None, self._buf.numel(), ctypes.byref(n), ctypes.byref(tot),
                                           ctypes.byref(mx), ctypes.byref(ck))
        if rc:
            raise ZstdError(rc, "cuda_zstd_seekable_info")
        self.num_frames, self.size, self.max_frame, self.has_checksums = n.value, tot.value, mx.value, bool(ck.value)
        self._temp = None

    def _read(self, offset: int, length: int, verify: bool, jobs: int, stream):
        torch = _torch()
        need = lib().cuda_zstd_seekable_read_get_temp_size_jobs(self.num_frames, jobs, self.max_frame)
        if self._temp is None or self._temp.numel() < need:
            self._temp = None
            self._temp = torch.empty(need, dtype=torch.uint8, device=self._buf.device)
        out = torch.empty(max(length, 1), dtype=torch.uint8, device=self._buf.device)
        written = ctypes.c_size_t(0)
        rc = lib().cuda_zstd_seekable_read(self._mgr._h, self._buf.data_ptr(), self._buf.numel(), offset, length, out.data_ptr(),
                                           ctypes.byref(written), 1 if verify else 0, self._temp.data_ptr(), self._temp.numel(),
                                           _stream_ptr(stream))
        return rc, out[: written.value]

    def read(self, offset: int, length: int, verify: bool = False, stream=None):
        """Bytes [offset, offset + length) of the content.  Only the frames that cover the range
        are decoded; verify=True checks them against the table's checksums (when it has them)."""
        if offset < 0 or length < 0:
            raise ZstdError(INVALID, "SeekableReader.read")
        # temp for the frames an evenly split stream would touch; the full table's on TOO_SMALL
        avg = max(1, self.size // max(self.num_frames, 1))
        jobs = min(self.num_frames, 4 * (length // avg + 2))
        rc, out = self._read(offset, length, verify, jobs, stream)
        if rc == TOO_SMALL and jobs < self.num_frames:
            rc, out = self._read(offset, length, verify, self.num_frames, stream)
        if rc:
            raise ZstdError(rc, "cuda_zstd_seekable_read")
        return _host_bytes(out) if self._host else out

    def read_all(self, verify: bool = False, stream=None):
        return self.read(0, self.size, verify, stream)

    def read_ranges(self, offsets, lengths, verify: bool = False, stream=None, raise_on_error: bool = True):
        """Many ranges in one device call (cuda_zstd_seekable_read_ranges): the table is scanned
        once and a frame that several ranges touch is decoded once.  offsets, lengths: sequences
        of ints or CUDA int64 tensors (the offsets then never leave the device).  Returns one
        view per range of a packed device buffer, range i at the sum of the earlier lengths (a
        list of bytes from a reader over host bytes).  A failed range (past the content, or over
        a frame that does not decode or verify) raises ZstdError with the first such range's
        code; with raise_on_error=False the result is (list, statuses), statuses an int32 host
        tensor, and a failed range's bytes are unspecified."""
        torch = _torch()
        dev = self._buf.device
        s = stream if stream is not None else torch.cuda.current_stream()
        if len(lengths) == 0 and len(offsets) == 0:
            return [] if raise_on_error else ([], torch.zeros(0, dtype=torch.int32))
        with torch.cuda.stream(s):
            d_off = offsets.to(torch.int64).contiguous() if _is_cuda_tensor(offsets) else \
                torch.tensor([int(v) for v in offsets], dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
            if _is_cuda_tensor(lengths):
                d_len = lengths.to(torch.int64).contiguous()
                lens = [int(v) for v in d_len.cpu()]  # the views are cut on the host: waits for the lengths
            else:
                lens = [int(v) for v in lengths]
                d_len = torch.tensor(lens, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
            r = len(lens)
            if d_off.numel() != r or any(v < 0 for v in lens):
                raise ZstdError(INVALID, "SeekableReader.read_ranges")
            total, max_length = sum(lens), max(lens)
            out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
            d_ptrs = out.data_ptr() + torch.cumsum(d_len, 0) - d_len  # range i at the sum of the earlier lengths
            statuses = torch.zeros(r, dtype=torch.int32, device=dev)
            # temp for the frames an evenly split stream would touch; the full table's on TOO_SMALL
            avg = max(1, self.size // max(self.num_frames, 1))
            jobs = min(self.num_frames, total // avg + 2 * r)
            while True:
                need = lib().cuda_zstd_seekable_read_ranges_get_temp_size(self.num_frames, r, jobs, self.max_frame)
                if self._temp is None or self._temp.numel() < need:
                    self._temp = None
                    self._temp = torch.empty(need, dtype=torch.uint8, device=dev)
                for t in (self._buf, self._temp, d_off, d_len):
                    t.record_stream(s)
                rc = lib().cuda_zstd_seekable_read_ranges(self._mgr._h, self._buf.data_ptr(), self._buf.numel(), d_off.data_ptr(), d_len.data_ptr(),
                                                          d_ptrs.data_ptr(), r, max_length, 1 if verify else 0, statuses.data_ptr(), None,
                                                          self._temp.data_ptr(), self._temp.numel(), s.cuda_stream)
                if rc != TOO_SMALL or jobs >= self.num_frames:
                    break
                jobs = self.num_frames
            if rc:
                raise ZstdError(rc, "cuda_zstd_seekable_read_ranges")
            st = statuses.cpu()  # (the call has waited for the stream)
            host = out.cpu() if self._host else None
        if raise_on_error and bool(st.any()):
            raise ZstdError(int(st[st != 0][0]), "cuda_zstd_seekable_read_ranges")
        starts = [0] * r
        for k in range(1, r):
            starts[k] = starts[k - 1] + lens[k - 1]
        if self._host:
            hb = host.numpy().tobytes()
            views = [hb[a:a + n] for a, n in zip(starts, lens)]
        else:
            views = [out[a:a + n] for a, n in zip(starts, lens)]
        return views if raise_on_error else (views, st)

    @classmethod
    def from_frames(cls, data, manager=None, max_frames: int = None, stream=None) -> "SeekableReader":
        """A reader over concatenated frames that carry no seek table (pzstd output, joined .zst
        files, frames written back to back): seekable_index builds the table on the device.
        `manager` also decodes the frames, so its dictionary serves both."""
        r = cls(seekable_index(data, max_frames, manager, stream), manager)
        r._host = _is_host(data)
        return r


def seekable_index(data, max_frames: int = None, decoder=None, stream=None):
    """Concatenated Zstandard (and skippable) frames -> a uint8 device tensor holding the same
    bytes followed by their seek table (cuda_zstd_seekable_index): a seekable stream for
    SeekableReader and for stock zstd.  One device copy of the stream into a buffer with room; the
    frames are found and the table is written on the device.  max_frames bounds the table (None:
    a guess from the size, and a second call with the stream's own count if it was too low).
    decoder: a BatchedDecompressor / BatchedCompressor whose dictionary or dictionary set sizes
    frames that state no content size.  A malformed stream raises ZstdError, with the complete
    frames before the failing one in .num_frames and its offset in .error_offset."""
    torch = _torch()
    src = _to_device(data) if _is_host(data) else data.contiguous().view(torch.uint8).reshape(-1)
    size = src.numel()
    if size == 0 or (max_frames is not None and max_frames < 0):
        raise ZstdError(INVALID, "seekable_index")
    n = max(1024, size // 4096) if max_frames is None else int(max_frames)
    s = stream if stream is not None else torch.cuda.current_stream()
    tb, nf, eo = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_ulonglong(0)
    with torch.cuda.stream(s):
        while True:
            cap = 17 + 8 * n
            buf = torch.empty(size + cap, dtype=torch.uint8, device=src.device)
            buf[:size].copy_(src)
            temp = torch.empty(lib().cuda_zstd_seekable_index_get_temp_size(size, n), dtype=torch.uint8, device=src.device)
            rc = lib().cuda_zstd_seekable_index(decoder._h if decoder is not None else None, buf.data_ptr(), size, n, buf.data_ptr() + size, cap,
                                                ctypes.byref(tb), ctypes.byref(nf), ctypes.byref(eo), temp.data_ptr(), temp.numel(), s.cuda_stream)
            if rc == TOO_SMALL and max_frames is None and nf.value > n:
                n = nf.value
                continue
            break
    if rc:
        e = ZstdError(rc, "cuda_zstd_seekable_index")
        e.num_frames, e.error_offset = nf.value, eo.value
        raise e
    return buf[: size + tb.value]


def decompress_frames(data, decoder=None, stream=None):
    """Decode concatenated frames frame-parallel: seekable_index, then one read of everything.
    Host input gives bytes back, a device tensor a device tensor."""
    return SeekableReader.from_frames(data, decoder, stream=stream).read_all(stream=stream)


# Adaptive level selection (cuda_zstd_adaptive_*; reference adaptive::AdaptiveLevelSelector,
# include/cuda_zstd_adaptive.h): which level a chunk is worth, from statistics of its first
# sample_bytes bytes and the reference's decision tree.
SPEED, BALANCED, RATIO = 0, 1, 2  # AdaptivePreference
HAS_PATTERNS, IS_RANDOM = 1, 2  # bits of a statistics record's flags


class AdaptiveStats(ctypes.Structure):
    """cuda_zstd_adaptive_stats_t."""
    _fields_ = [("sample_size", ctypes.c_uint), ("repeated_pairs", ctypes.c_uint), ("max_run_length", ctypes.c_uint),
                ("pattern_score", ctypes.c_uint), ("unique_bytes", ctypes.c_uint), ("flags", ctypes.c_uint), ("entropy", ctypes.c_float),
                ("repetition_ratio", ctypes.c_float), ("compressibility", ctypes.c_float), ("level", ctypes.c_int)]


def _stats_dict(s: AdaptiveStats) -> dict:
    d = {name: getattr(s, name) for name, _ in AdaptiveStats._fields_}
    d["has_patterns"], d["is_random"] = bool(s.flags & HAS_PATTERNS), bool(s.flags & IS_RANDOM)
    return d


def adaptive_stats_numpy(stats):
    """The stats tensor of analyze_batch as a structured numpy array, one record per chunk, with
    the fields of cuda_zstd_adaptive_stats_t (copies to the host: waits for the device)."""
    import numpy as np

    dt = np.dtype([(name, {ctypes.c_uint: "<u4", ctypes.c_float: "<f4", ctypes.c_int: "<i4"}[t]) for name, t in AdaptiveStats._fields_])
    return stats.cpu().numpy().view(dt).reshape(-1)


def analyze_batch_device(d_ptrs, d_sizes, preference: int = BALANCED, sample_bytes: int = 65536, stream=None):
    """analyze_batch over device arrays (int64 tensors of chunk addresses and sizes): one
    stream-ordered launch for the whole batch (cuda_zstd_adaptive_analyze_batch_async)."""
    torch = _torch()
    n = d_ptrs.numel()
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):  # the outputs and the temp buffer are ordered on the same stream
        levels = torch.empty(n, dtype=torch.int32, device=d_ptrs.device)
        stats = torch.empty(n * ctypes.sizeof(AdaptiveStats), dtype=torch.uint8, device=d_ptrs.device)
        temp = torch.empty(max(lib().cuda_zstd_adaptive_get_temp_size(n), 4), dtype=torch.uint8, device=d_ptrs.device)
        rc = lib().cuda_zstd_adaptive_analyze_batch_async(d_ptrs.data_ptr(), d_sizes.data_ptr(), n, sample_bytes, preference, stats.data_ptr(),
                                                          levels.data_ptr(), temp.data_ptr(), temp.numel(), s.cuda_stream)
    if rc:
        raise ZstdError(rc, "cuda_zstd_adaptive_analyze_batch_async")
    return levels, stats


def analyze_batch(chunks: Sequence, preference: int = BALANCED, sample_bytes: int = 65536, stream=None):
    """Level and statistics of every chunk (uint8 device tensors) -> (levels, stats): an int32
    device tensor and a device byte tensor of cuda_zstd_adaptive_stats_t records
    (adaptive_stats_numpy reads them).  Nothing waits for the device: the chunk addresses go up
    from pinned memory, and the results are valid in stream order."""
    torch = _torch()
    ins = [c.contiguous().view(torch.uint8) for c in chunks]
    n = len(ins)
    s = stream if stream is not None else torch.cuda.current_stream()
    table = torch.tensor([[t.data_ptr() for t in ins], [t.numel() for t in ins]], dtype=torch.int64).reshape(2, n)
    with torch.cuda.stream(s):
        d_table = table.pin_memory().to("cuda", non_blocking=True)
        for t in ins:
            t.record_stream(s)
    return analyze_batch_device(d_table[0], d_table[1], preference, sample_bytes, s)


def select_level(data, preference: int = BALANCED, sample_bytes: int = 65536, stream=None) -> dict:
    """cuda_zstd_adaptive_select_level on one buffer (a device tensor, or host bytes / numpy,
    which are uploaded): the fields of cuda_zstd_adaptive_stats_t, `level` among them, plus
    has_patterns / is_random.  Waits for the result."""
    torch = _torch()
    t = _to_device(data) if _is_host(data) else data.contiguous().view(torch.uint8)
    out = AdaptiveStats()
    rc = lib().cuda_zstd_adaptive_select_level(t.data_ptr() if t.numel() else None, t.numel(), sample_bytes, preference, ctypes.byref(out),
                                               _stream_ptr(stream))
    if rc:
        raise ZstdError(rc, "cuda_zstd_adaptive_select_level")
    return _stats_dict(out)


def is_compressible(data):
    """(compressible, estimated_ratio): compressibility > 0.3 and 1 + 3 * compressibility
    (reference adaptive::is_compressible)."""
    c = select_level(data)["compressibility"]
    return c > 0.3, 1.0 + 3.0 * c


def adaptive_finalize_host(hist, repeated_pairs: int, max_run_length: int, pattern_score: int, preference: int = BALANCED) -> dict:
    """The derived values and the level from integer statistics, on the host
    (cuda_zstd_adaptive_finalize_host: the function the device runs); needs no GPU."""
    h = (ctypes.c_uint * 256)(*[int(v) for v in hist])
    out = AdaptiveStats()
    rc = lib().cuda_zstd_adaptive_finalize_host(h, sum(h), repeated_pairs, max_run_length, pattern_score, preference, ctypes.byref(out))
    if rc:
        raise ZstdError(rc, "cuda_zstd_adaptive_finalize_host")
    return _stats_dict(out)


def _one_call_batch(what: str, handle, ins, *, slot: int, rows: dict, index=None, record, temp_bytes: int, call, host: bool, stream) -> List:
    """The batched one-call functions below, after their argument checks: one pinned int64 table of
    named rows ("in": the inputs' addresses, "in_size", "out": the output slots, then `rows`), sizes,
    statuses and temp, call(t, d_index, d_sizes, d_status, temp, stream) with t[name] the device row,
    and one stacked copy back, the single wait; then `handle` is closed and `out` sliced by slot.
    index: None, a device int32 tensor, or ints that go up from pinned memory.  record: the tensors
    the call reads."""
    torch = _torch()
    n, s = len(ins), stream
    with torch.cuda.stream(s):
        out = torch.empty(n * slot, dtype=torch.uint8, device="cuda")
        host_rows = {"in": [t.data_ptr() if t.numel() else 0 for t in ins], "in_size": [t.numel() for t in ins],
                     "out": [out.data_ptr() + k * slot for k in range(n)], **rows}
        d_table = torch.tensor(list(host_rows.values()), dtype=torch.int64).pin_memory().to("cuda", non_blocking=True)
        t = dict(zip(host_rows, d_table))
        if index is not None and not _is_cuda_tensor(index):
            index = torch.tensor(index, dtype=torch.int32).pin_memory().to("cuda", non_blocking=True)
        if s != torch.cuda.current_stream():  # (the inputs' allocator stream is the current one)
            for r in record:
                r.record_stream(s)
        d_sizes = torch.empty(n, dtype=torch.int64, device="cuda")
        d_status = torch.empty(n, dtype=torch.int32, device="cuda")
        temp = torch.empty(temp_bytes, dtype=torch.uint8, device="cuda")
        call(t, index, d_sizes, d_status, temp, s)
        got_sizes, got_status = torch.stack([d_sizes, d_status.to(torch.int64)]).cpu().tolist()  # the one wait (stream-ordered copy)
    handle.close()
    res = []
    for k in range(n):
        if got_status[k] != OK:
            raise ZstdError(got_status[k], f"{what} item {k}")
        f = out[k * slot : k * slot + got_sizes[k]]
        res.append(_host_bytes(f) if host else f)
    return res


def _slot(nbytes: int) -> int:
    return ((nbytes + 255) // 256) * 256


def _uploaded(items, torch):
    return [(_to_device(c) if _is_host(c) else c).contiguous().view(torch.uint8) for c in items]


def compress_batch_levels(chunks: Sequence, levels, checksum: bool = False, stream=None) -> List:
    """Compress chunk i (uint8 device tensors) at levels[i] in one stream-ordered call
    (nvcomp_zstd_batched_compress_levels_async_v5) -> the frames in input order, each the bytes
    Manager(levels[i]) writes for it.  levels: a device int32 tensor, read on the device in stream
    order and never copied to the host, or a sequence of ints.  Waits once, for the frames' sizes;
    a chunk whose level is outside 1..22 raises ZstdError."""
    torch = _torch()
    n = len(chunks)
    if n == 0:
        return []
    s = stream if stream is not None else torch.cuda.current_stream()
    ins = [c.contiguous().view(torch.uint8) for c in chunks]
    max_chunk = max(max(t.numel() for t in ins), 1)
    if _is_cuda_tensor(levels):
        with torch.cuda.stream(s):
            levels = levels.to(torch.int32).contiguous()
    else:
        levels = [int(v) for v in levels]
    if (levels.numel() if _is_cuda_tensor(levels) else len(levels)) != n:
        raise ZstdError(INVALID, "compress_batch_levels: one level per chunk")
    bc = BatchedCompressor(3, checksum=checksum)  # (the level of the handle is not used)
    return _one_call_batch("compress_batch_levels", bc, ins, slot=_slot(max_compressed_size(max_chunk)), rows={}, index=levels, record=ins,
                           temp_bytes=bc.temp_size_levels(n, max_chunk), host=False, stream=s,
                           call=lambda t, lv, sz, st, temp, s: bc.compress_levels_async(t["in"], t["in_size"], lv, max_chunk, t["out"], sz, st, temp, s))


def _prefix_table(items, prefixes, torch):
    """Device tensors of the items and their prefixes (hosts are uploaded; None: no prefix), and
    the prefixes' table rows."""
    ins = _uploaded(items, torch)
    if len(prefixes) != len(ins):
        raise ZstdError(INVALID, "one prefix (or None) per item")
    pre = [None if p is None else _uploaded([p], torch)[0] for p in prefixes]
    return ins, [p for p in pre if p is not None], {"pre": [0 if p is None or not p.numel() else p.data_ptr() for p in pre],
                                                    "pre_size": [0 if p is None else p.numel() for p in pre]}


def compress_batch_prefix(chunks: Sequence, prefixes: Sequence, level: int = 3, checksum: bool = False, stream=None) -> List:
    """Compress chunk i behind prefixes[i] (the bytes that precede it: a raw-content dictionary;
    None = no prefix) in one stream-ordered call (nvcomp_zstd_batched_compress_prefix_async_v5) ->
    the frames in input order.  Hosts (bytes, numpy) or CUDA tensors in; device tensors in ->
    device tensors out, hosts in -> bytes out.  Waits once, for the frames' sizes."""
    torch = _torch()
    n = len(chunks)
    if n == 0:
        return []
    s = stream if stream is not None else torch.cuda.current_stream()
    ins, pre, rows = _prefix_table(chunks, prefixes, torch)
    max_chunk = max(max(t.numel() for t in ins), 1)
    bc = BatchedCompressor(level, checksum=checksum)
    return _one_call_batch("compress_batch_prefix", bc, ins, slot=_slot(bc.max_out(max_chunk)), rows=rows, record=ins + pre,
                           temp_bytes=bc.temp_size_prefix(n, max_chunk), host=_is_host(chunks[0]), stream=s,
                           call=lambda t, _, sz, st, temp, s: bc.compress_prefix_async(t["in"], t["in_size"], t["pre"], t["pre_size"], max_chunk, t["out"],
                                                                                       sz, st, temp, s))


def decompress_batch_prefix(frames: Sequence, prefixes: Sequence, capacities=None, stream=None) -> List:
    """Decode frame i behind prefixes[i] (None = no prefix) in one stream-ordered call
    (nvcomp_zstd_batched_decompress_prefix_async_v5).  capacities: one output capacity per frame
    (default: the frame header's content size).  Hosts in -> bytes out, CUDA tensors in -> tensors."""
    torch = _torch()
    n = len(frames)
    if n == 0:
        return []
    s = stream if stream is not None else torch.cuda.current_stream()
    ins, pre, rows = _prefix_table(frames, prefixes, torch)
    caps = [int(c) for c in capacities] if capacities is not None else [_frame_size(t) for t in ins]
    max_out = max(max(caps), 1)
    bd = BatchedDecompressor()
    return _one_call_batch("decompress_batch_prefix", bd, ins, slot=_slot(max_out), rows={"cap": caps, **rows}, record=ins + pre,
                           temp_bytes=bd.temp_size(n, max_out), host=_is_host(frames[0]), stream=s,
                           call=lambda t, _, sz, st, temp, s: bd.decompress_prefix_async(t["in"], t["in_size"], t["pre"], t["pre_size"], t["cap"], max_out,
                                                                                         t["out"], sz, st, temp, s))


def compress_batch_dicts(chunks: Sequence, dict_set: "DictionarySet", indices: Sequence[int], level: int = 3, checksum: bool = False,
                         dict_entropy: bool = False, stream=None) -> List:
    """Compress chunk i against entry indices[i] of dict_set (-1: no dictionary) in one
    stream-ordered call (nvcomp_zstd_batched_compress_dicts_async_v5) -> the frames in input order,
    each what a handle with that one dictionary set writes.  Hosts (bytes, numpy) or CUDA tensors
    in; device tensors in -> device tensors out, hosts in -> bytes out.  Waits once, for the sizes."""
    torch = _torch()
    n = len(chunks)
    if n == 0:
        return []
    if len(indices) != n:
        raise ZstdError(INVALID, "one entry index (or -1) per chunk")
    s = stream if stream is not None else torch.cuda.current_stream()
    ins = _uploaded(chunks, torch)
    max_chunk = max(max(t.numel() for t in ins), 1)
    bc = BatchedCompressor(level, checksum=checksum, dict_entropy=dict_entropy)
    bc.set_dictionary_set(dict_set)
    return _one_call_batch("compress_batch_dicts", bc, ins, slot=_slot(bc.max_out(max_chunk)), rows={}, index=[int(i) for i in indices], record=ins,
                           temp_bytes=bc.temp_size_dicts(n, max_chunk), host=_is_host(chunks[0]), stream=s,
                           call=lambda t, ix, sz, st, temp, s: bc.compress_dicts_async(t["in"], t["in_size"], ix, max_chunk, t["out"], sz, st, temp, s))


def decompress_batch_dicts(frames: Sequence, dict_set: "DictionarySet", indices: Sequence[int] = None, capacities=None, stream=None) -> List:
    """Decode frame i against dict_set in one stream-ordered call
    (nvcomp_zstd_batched_decompress_dicts_async_v5): every frame's dictionary is resolved on the
    device from its Dictionary_ID, or is entry indices[i] where that is >= 0 (the way to name a
    raw-content entry).  capacities: one output capacity per frame (default: the frame header's
    content size).  Hosts in -> bytes out, CUDA tensors in -> tensors."""
    torch = _torch()
    n = len(frames)
    if n == 0:
        return []
    if indices is not None and len(indices) != n:
        raise ZstdError(INVALID, "one entry index (or -1) per frame")
    s = stream if stream is not None else torch.cuda.current_stream()
    ins = _uploaded(frames, torch)
    caps = [int(c) for c in capacities] if capacities is not None else [_frame_size(t) for t in ins]
    max_out = max(max(caps), 1)
    bd = BatchedDecompressor()
    bd.set_dictionary_set(dict_set)
    return _one_call_batch("decompress_batch_dicts", bd, ins, slot=_slot(max_out), rows={"cap": caps},
                           index=None if indices is None else [int(i) for i in indices], record=ins, temp_bytes=bd.temp_size(n, max_out),
                           host=_is_host(frames[0]), stream=s,
                           call=lambda t, ix, sz, st, temp, s: bd.decompress_dicts_async(t["in"], t["in_size"], ix, t["cap"], max_out, t["out"], sz, st, temp, s))


def compress_batch_adaptive(chunks: Sequence, preference: int = BALANCED, stream=None):
    """Compress every chunk (uint8 device tensors) at the level the selector gives it ->
    (frames, levels): one analysis of the batch, then one compress_batch_levels call fed the
    analysis' device tensor on the same stream; the levels are copied to the host only for the
    return value.  Frames in input order."""
    d_levels = analyze_batch(chunks, preference, stream=stream)[0]
    frames = compress_batch_levels(chunks, d_levels, stream=stream)
    return frames, [int(v) for v in d_levels.cpu()]


def hybrid_compress(data, level: int = 3) -> bytes:
    return HybridEngine(level).compress(data)


def hybrid_decompress(data) -> bytes:
    return HybridEngine(3).decompress(data)


def validate_compressed_data(data, check_checksum: bool = True) -> bool:
    """Frame-header validation (reference validate_compressed_data_py): True iff the buffer
    starts with (skippable frames and) a parseable zstd frame header."""
    try:
        extract_metadata(data)
        return True
    except ZstdError:
        return False


def estimate_compressed_size(uncompressed_size: int, level: int = 3) -> int:
    return max_compressed_size(uncompressed_size)


def is_cuda_available() -> bool:
    """True when a GPU is visible (the reference's name; here an MI355X through ROCm)."""
    import torch

    return torch.cuda.is_available()


def get_cuda_device_info(device: int = 0) -> dict:
    torch = _torch()
    p = torch.cuda.get_device_properties(device)
    return {"name": p.name, "total_memory": p.total_memory, "multi_processor_count": p.multi_processor_count,
            "gcn_arch_name": getattr(p, "gcnArchName", None), "device": device}


def metadata_frame(level: int) -> bytes:
    """The 16-byte skippable metadata frame recording `level` (cuda_zstd_write_metadata_frame)."""
    buf = ctypes.create_string_buffer(16)
    n = ctypes.c_size_t()
    rc = lib().cuda_zstd_write_metadata_frame(buf, 16, level, ctypes.byref(n), None)
    if rc:
        raise ZstdError(rc, "cuda_zstd_write_metadata_frame")
    return buf.raw[: n.value]


def extract_metadata(data) -> dict:
    """Header fields of the first zstd frame after any skippable frames (host bytes or a
    device tensor): level (from a metadata frame, else 3), content size, dictionary ID, checksum."""
    if isinstance(data, (bytes, bytearray, memoryview)):
        b = bytes(data)
        ptr, keep = ctypes.create_string_buffer(b, max(len(b), 1)), None
        n = len(b)
    else:
        keep, ptr, n = data, data.data_ptr(), data.numel()
    lv, us, did, ck = ctypes.c_uint(), ctypes.c_ulonglong(), ctypes.c_uint(), ctypes.c_int()
    rc = lib().cuda_zstd_extract_metadata(ptr, n, ctypes.byref(lv), ctypes.byref(us), ctypes.byref(did), ctypes.byref(ck))
    del keep
    if rc:
        raise ZstdError(rc, "cuda_zstd_extract_metadata")
    return {"level": lv.value, "uncompressed_size": us.value, "dictionary_id": did.value, "checksum": bool(ck.value)}


def profile_enable(on: bool = True) -> None:
    """Record HIP events around each kernel of every launch (on the launch stream)."""
    lib().cuda_zstd_hip_profile_enable(1 if on else 0)


def profile_collect():
    """-> (launches, [ms_lz, ms_entropy, ms_gather] summed over them)."""
    ms = (ctypes.c_double * 3)()
    n = lib().cuda_zstd_hip_profile_collect(ms)
    return n, list(ms)

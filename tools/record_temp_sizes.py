#!/usr/bin/env python3
"""Record what every public compress and decode temp-size query of the library returns into
tests/golden/temp_sizes.json (tests/test_temp_sizes.py and tests/test_gpu_plan_routes.py compare
against it).  Run it with the library of the commit whose sizes are the reference
(CUDA_ZSTD_HIP_LIB selects another build).  It reads nothing but the library.

  python tools/record_temp_sizes.py          the dictionary-less entries, compress and decode (no GPU
                                             needed); merges into the file
  python tools/record_temp_sizes.py --dict   adds the entries of a handle with a dictionary set
                                             (setting one needs a device); merges into the file
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "custom-nvcomp-with-zstd_amd"))
OUT = os.path.join(ROOT, "tests", "golden", "temp_sizes.json")

LEVELS = [1, 3, 4, 5, 9, 22]
SHAPES = [(1, 1), (1, 32768), (1, 32769), (16, 65536), (16, 65537), (8, 163840), (16384, 65536)]
FRAMES = [1, 65536, 65537, 1 << 20, 64 << 20]
# tests/test_gpu_plan_routes.py: its batch, its dictionary's size and the levels it sets one at
ROUTE_SIZES = [1, 32767, 32768, 32769, 65536, 65537, 98305, 163840]
DICT_BYTES = 40 * 1024
# the decode-side queries: counts and output capacities on both sides of the decoder slot's 64-byte
# floor and 128 KiB cap
DEC_COUNTS = [1, 2, 2049]
DEC_CAPS = [1, 63, 64, 65, 131072, 131073]
DEC_RANGES = 3  # ranges of a batched seekable read
DICT_LEVELS = [3, 5]


def sizes_of(L):
    """Every dictionary-less entry: {entry: {level: {shape: bytes}}} (the static entry has no level)."""
    key = lambda n, m: f"{n}x{m}"
    arr = lambda v: (ctypes.c_size_t * len(v))(*v)
    out = {"batch_workspace": {}, "batched_temp": {}, "batch_compress_temp": {}, "single": {}, "single_ldm": {}}
    out["levels_temp"] = {key(n, m): L.nvcomp_zstd_batched_compress_levels_get_temp_size_v5(n, m) for n, m in SHAPES}
    for lv in LEVELS:
        m = L.cuda_zstd_create_manager(lv)
        h = L.nvcomp_zstd_batch_create_v5(lv, 65536, 0)
        out["batch_workspace"][str(lv)] = {key(n, c): L.cuda_zstd_get_batch_compress_workspace_size(m, arr([c] * n), n) for n, c in SHAPES}
        out["batch_workspace"][str(lv)]["routes"] = L.cuda_zstd_get_batch_compress_workspace_size(m, arr(ROUTE_SIZES), len(ROUTE_SIZES))
        out["batched_temp"][str(lv)] = {key(n, c): L.nvcomp_zstd_batch_get_batched_temp_size_v5(h, n, c) for n, c in SHAPES}
        out["batch_compress_temp"][str(lv)] = {key(n, c): L.nvcomp_zstd_batch_get_compress_temp_size_v5(h, arr([c] * n), n) for n, c in SHAPES}
        out["batch_compress_temp"][str(lv)]["routes"] = L.nvcomp_zstd_batch_get_compress_temp_size_v5(h, arr(ROUTE_SIZES), len(ROUTE_SIZES))
        out["single"][str(lv)] = {str(n): L.cuda_zstd_get_compress_workspace_size(m, n) for n in FRAMES}
        assert L.cuda_zstd_set_long_distance(m, 1, 0, 0) == 0
        out["single_ldm"][str(lv)] = {str(n): L.cuda_zstd_get_compress_workspace_size(m, n) for n in FRAMES}
        L.nvcomp_zstd_batch_destroy_v5(h)
        L.cuda_zstd_destroy_manager(m)
    return out


def decode_sizes_of(L):
    """The decode-side entries (no level: the decoder's workspace has none): {entry: {shape: bytes}}.
    dec_single, dec_batch_workspace and dec_batch_temp size for 128 KiB blocks whatever the capacity
    (they pin that and the count); the other three follow the capacity across the slot's 64-byte floor
    and 128 KiB cap."""
    key = lambda n, m: f"{n}x{m}"
    arr = lambda v: (ctypes.c_size_t * len(v))(*v)
    shapes = [(n, c) for n in DEC_COUNTS for c in DEC_CAPS]
    m = L.cuda_zstd_create_manager(3)
    h = L.nvcomp_zstd_batch_create_v5(3, 65536, 0)
    out = {
        "dec_single": {str(c): L.cuda_zstd_get_decompress_workspace_size(m, c) for c in DEC_CAPS},
        "dec_batch_workspace": {key(n, c): L.cuda_zstd_get_batch_decompress_workspace_size(m, arr([c] * n), n) for n, c in shapes},
        "dec_batch_temp": {key(n, c): L.nvcomp_zstd_batch_get_decompress_temp_size_v5(h, arr([c] * n), n) for n, c in shapes},
        "dec_batched_temp": {key(n, c): L.nvcomp_zstd_batched_decompress_get_temp_size_v5(n, c) for n, c in shapes},
        "seek_read_temp": {key(n, c): L.cuda_zstd_seekable_read_get_temp_size(n, c) for n, c in shapes},
        "seek_ranges_temp": {key(n, c): L.cuda_zstd_seekable_read_ranges_get_temp_size(n, DEC_RANGES, n, c) for n, c in shapes},
    }
    L.nvcomp_zstd_batch_destroy_v5(h)
    L.cuda_zstd_destroy_manager(m)
    return out


def dict_sizes_of():
    """{level: bytes}: BatchedCompressor.temp_size(len(ROUTE_SIZES), max(ROUTE_SIZES)) with a raw
    DICT_BYTES dictionary set (the size depends on the dictionary only through "has one")."""
    import cuda_zstd

    d = cuda_zstd.Dictionary.load(bytes(range(256)) * (DICT_BYTES // 256))
    out = {}
    for lv in DICT_LEVELS:
        c = cuda_zstd.BatchedCompressor(lv, 65536)
        c.set_dictionary(d)
        out[str(lv)] = c.temp_size(len(ROUTE_SIZES), max(ROUTE_SIZES))
        c.close()
    return out


def main():
    import cuda_zstd

    if "--dict" in sys.argv[1:]:
        with open(OUT) as f:
            doc = json.load(f)
        doc["dict_batched_temp"] = dict_sizes_of()
    else:
        doc = {}
        if os.path.exists(OUT):  # (the --dict entries stay)
            with open(OUT) as f:
                doc = json.load(f)
        doc.update(sizes_of(cuda_zstd.lib()))
        doc.update(decode_sizes_of(cuda_zstd.lib()))
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Seekable-stream timings on bench.py's C3 workload (16,384 x 64 KiB mix chunks, level 3).

  (a) pack (cuda_zstd_seekable_pack_async) without and with checksums: milliseconds, as a
      fraction of the C3 compress step of the same run, and as a ratio to a hipMemcpyAsync
      device-to-device copy of the stream's bytes (the floor for any copy);
  (b) read_all (cuda_zstd_seekable_read of the whole content) against the batched decode of the
      same frames from their separate slots (same decoder: the ceiling) and against
      Manager.decompress of a stream as one item (one workgroup walks the frames serially; timed
      on a prefix of --single-item-frames frames, its rate does not depend on the length);
  (c) a 1 MiB read at an odd offset in the middle of the stream.

Pack and the batched decode are timed with events on the launch stream; the reads block, so they
(and the batched decode once more, for a like-for-like figure) are timed on the host clock around
a device synchronise.  Writes one JSON object to --out and prints it on one line.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "custom-nvcomp-with-zstd_amd"))

CHUNK = 65536
SEED = 0x5EED0003


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--single-item-frames", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seekable_bench.json"))
    a = ap.parse_args()

    import torch

    import cuda_zstd
    import zh_testlib as T

    L = cuda_zstd.lib()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    dev = torch.device("cuda:0")
    n = a.chunks
    host = T.gen(T.DG_MIX, n, SEED, CHUNK)
    d_in = torch.from_numpy(host).to(dev)
    bc = cuda_zstd.BatchedCompressor(3, CHUNK)
    slot = (bc.max_out(CHUNK) + 255) // 256 * 256
    slots = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    in_ptrs, f_ptrs = d_in.data_ptr() + ar * CHUNK, slots.data_ptr() + ar * slot
    in_sizes = torch.full((n,), CHUNK, dtype=torch.int64, device=dev)
    f_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    f_status = torch.zeros(n, dtype=torch.int32, device=dev)
    temp = torch.empty(max(bc.temp_size(n, CHUNK), bc.pack_temp_size(n), 256), dtype=torch.uint8, device=dev)
    cap = bc.seekable_max_size(n, slot, True)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_size = torch.zeros(1, dtype=torch.int64, device=dev)
    d_status = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)

    def events(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / a.steps

    def wall(fn, steps=None, warmup=None):
        for _ in range(a.warmup if warmup is None else warmup):
            fn()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps or a.steps):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3 / (steps or a.steps)

    def compress():
        bc.compress_async(in_ptrs, in_sizes, CHUNK, f_ptrs, f_sizes, f_status, temp, stream)

    def pack(ck, count=n, dst=out):
        bc.pack_seekable_async(f_ptrs[:count], f_sizes[:count], f_status[:count], in_ptrs[:count], in_sizes[:count], slot, dst, d_size, d_status,
                               temp, ck, stream)

    ms_compress = events(compress)
    assert bool((f_status == 0).all().item())
    ms_pack = events(lambda: pack(False))
    size_plain = int(d_size.item())
    ms_pack_ck = events(lambda: pack(True))
    size_ck = int(d_size.item())
    assert int(d_status.item()) == 0 and size_ck == size_plain + 4 * n
    print(f"compress {ms_compress:.3f} ms, pack {ms_pack:.3f} ms, pack+checksums {ms_pack_ck:.3f} ms", flush=True)
    src = torch.empty(size_ck, dtype=torch.uint8, device=dev)
    ms_memcpy = events(lambda: hip.hipMemcpyAsync(src.data_ptr(), out.data_ptr(), size_ck, 3, stream.cuda_stream))
    del src

    # (b) the checksummed stream is in `out`; decode it three ways
    total = n * CHUNK
    bd = cuda_zstd.BatchedDecompressor()
    back = torch.empty(total, dtype=torch.uint8, device=dev)
    back_ptrs = back.data_ptr() + ar * CHUNK
    dsizes = torch.zeros(n, dtype=torch.int64, device=dev)
    dstat = torch.full((n,), -1, dtype=torch.int32, device=dev)
    dtemp = torch.empty(max(bd.temp_size(n, CHUNK), 256), dtype=torch.uint8, device=dev)

    def batched():
        bd.decompress_async(f_ptrs, f_sizes, None, CHUNK, back_ptrs, dsizes, dstat, dtemp)

    ms_batched_ev = events(batched)
    ms_batched = wall(batched)
    assert torch.equal(back, d_in)
    del dtemp
    print(f"batched decode {ms_batched:.3f} ms", flush=True)

    rtemp = torch.empty(L.cuda_zstd_seekable_read_get_temp_size(n, CHUNK), dtype=torch.uint8, device=dev)
    written = ctypes.c_size_t(0)

    def read(off, length, verify=0):
        rc = L.cuda_zstd_seekable_read(bd._h, out.data_ptr(), size_ck, off, length, back.data_ptr(), ctypes.byref(written), verify,
                                       rtemp.data_ptr(), rtemp.numel(), stream.cuda_stream)
        assert rc == 0 and written.value == length, rc

    back.zero_()
    ms_read_all = wall(lambda: read(0, total))
    assert torch.equal(back, d_in)
    ms_read_all_verify = wall(lambda: read(0, total, 1))
    print(f"read_all {ms_read_all:.3f} ms, verified {ms_read_all_verify:.3f} ms", flush=True)

    # (c) 1 MiB at an odd offset in the middle
    off = total // 2 + 12345
    length = min(1 << 20, total - off)
    ms_read_1m = wall(lambda: read(off, length), steps=max(a.steps, 20))
    assert torch.equal(back[:length], d_in[off:off + length])
    print(f"1 MiB read {ms_read_1m:.3f} ms", flush=True)
    del rtemp

    # Manager.decompress of a stream as one item (a prefix: one workgroup decodes it serially)
    k = min(a.single_item_frames, n)
    pre = torch.empty(bc.seekable_max_size(k, slot, False), dtype=torch.uint8, device=dev)
    pack(False, k, pre)
    torch.cuda.synchronize(dev)
    pre_size = int(d_size.item())
    m = cuda_zstd.Manager(3)
    res = []

    def single():
        res[:] = [m.decompress(pre[:pre_size], k * CHUNK)]

    ms_single = wall(single, steps=1, warmup=1)
    assert torch.equal(res[0], d_in[: k * CHUNK])

    gbs = lambda nbytes, ms: round(nbytes / (ms / 1e3) / 1e9, 3)
    r = {
        "workload": f"C3: {n} x 64 KiB mix chunks (seed 0x5EED0003), level 3", "device": torch.cuda.get_device_name(0),
        "steps": a.steps, "warmup": a.warmup, "stream_bytes": size_plain, "stream_bytes_with_checksums": size_ck,
        "compress_ms": round(ms_compress, 3),
        "pack": {"ms": round(ms_pack, 3), "ms_with_checksums": round(ms_pack_ck, 3),
                 "fraction_of_compress": round(ms_pack / ms_compress, 4), "fraction_of_compress_with_checksums": round(ms_pack_ck / ms_compress, 4),
                 "memcpy_d2d_ms": round(ms_memcpy, 3), "ratio_to_memcpy": round(ms_pack / ms_memcpy, 2),
                 "ratio_to_memcpy_with_checksums": round(ms_pack_ck / ms_memcpy, 2),
                 "GBps_stream_bytes": gbs(size_plain, ms_pack), "timing": "events on the launch stream"},
        "read_all": {"ms": round(ms_read_all, 3), "GBps": gbs(total, ms_read_all), "ms_verify": round(ms_read_all_verify, 3),
                     "GBps_verify": gbs(total, ms_read_all_verify),
                     "batched_decode_separate_slots_ms": round(ms_batched, 3), "batched_decode_GBps": gbs(total, ms_batched),
                     "batched_decode_events_ms": round(ms_batched_ev, 3), "fraction_of_batched_decode_rate": round(ms_batched / ms_read_all, 3),
                     "single_item_frames": k, "single_item_ms": round(ms_single, 3), "single_item_GBps": gbs(k * CHUNK, ms_single),
                     "speedup_over_single_item": round(gbs(total, ms_read_all) / max(gbs(k * CHUNK, ms_single), 1e-9), 1),
                     "timing": "host clock around a device synchronise (the read blocks); decompressed bytes per second"},
        "read_1MiB": {"offset": off, "length": length, "ms": round(ms_read_1m, 3), "GBps": gbs(length, ms_read_1m),
                      "timing": "host clock, blocking call"},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(r, f, indent=1)
        f.write("\n")
    print(json.dumps(r))


if __name__ == "__main__":
    main()

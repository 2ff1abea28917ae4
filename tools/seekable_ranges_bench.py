#!/usr/bin/env python3
"""Batched range reads of a seekable stream against the route they replace, on the C3 stream of
tools/seekable_bench.py (16,384 x 64 KiB mix chunks, level 3, with checksums).

For R = 1, 64, 4,096 and 65,536 ranges of 4 KiB and R = 4,096 ranges of 256 B at seeded random
offsets: one cuda_zstd_seekable_read_ranges call against a loop of cuda_zstd_seekable_read over
the same ranges (the same build; both block, so both are timed on the host clock: medians of
--steps after --warmup, with min and max; a pass that takes over --long-pass-s seconds, the loop
at R = 65,536, is timed once and its entry says so).  frames_decoded is recorded next to R.  One
whole-stream range through the batched call against read_all shows what the staging copy costs;
read_all and the 1 MiB read of seekable_bench.py are recorded for comparison with
profiles/seekable_bench.json.  --resources: a JSON file of the zh_seek_* kernels' register, LDS
and scratch use in this build and its parent, copied into the result.
Writes one JSON object to --out and prints it on one line."""
import argparse
import ctypes
import json
import os
import statistics
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
    ap.add_argument("--long-pass-s", type=float, default=60.0)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seekable_ranges.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    import cuda_zstd
    import zh_testlib as T

    L = cuda_zstd.lib()
    dev = torch.device("cuda:0")
    n = a.chunks
    total = n * CHUNK
    d_in = torch.from_numpy(T.gen(T.DG_MIX, n, SEED, CHUNK)).to(dev)
    st = cuda_zstd.seekable_compress(d_in, frame_size=CHUNK, level=3, checksums=True)
    size = st.numel()
    bd = cuda_zstd.BatchedDecompressor()
    stream = torch.cuda.current_stream(dev).cuda_stream
    back = torch.zeros(total, dtype=torch.uint8, device=dev)
    rtemp = torch.empty(L.cuda_zstd_seekable_read_get_temp_size(n, CHUNK), dtype=torch.uint8, device=dev)
    written = ctypes.c_size_t(0)

    def once(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    def timed(fn):
        """Median, min and max of --steps passes after --warmup.  A pass longer than
        --long-pass-s (the loop of single reads at the largest R: minutes) is measured once,
        with no warm-up, and says so."""
        torch.cuda.synchronize(dev)
        first = once(fn)
        if first > a.long_pass_s * 1e3:
            return {"ms": round(first, 3), "min_ms": round(first, 3), "max_ms": round(first, 3), "steps": 1, "warmup": 0}
        for _ in range(a.warmup - 1):
            fn()
        torch.cuda.synchronize(dev)
        ms = [once(fn) for _ in range(a.steps)]
        return {"ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "steps": a.steps, "warmup": a.warmup}

    def read(off, length, dst):
        rc = L.cuda_zstd_seekable_read(bd._h, st.data_ptr(), size, off, length, dst, ctypes.byref(written), 0, rtemp.data_ptr(), rtemp.numel(), stream)
        assert rc == 0 and written.value == length, rc

    def batched(offs, lens, max_jobs):
        """(call, packed output, statuses, frames_decoded) for one batch of ranges"""
        r = len(offs)
        d_off = torch.tensor(offs, dtype=torch.int64).to(dev)
        d_len = torch.tensor(lens, dtype=torch.int64).to(dev)
        out = torch.zeros(sum(lens), dtype=torch.uint8, device=dev)
        d_ptr = out.data_ptr() + torch.cumsum(d_len, 0) - d_len
        d_st = torch.full((r,), -1, dtype=torch.int32, device=dev)
        temp = torch.empty(L.cuda_zstd_seekable_read_ranges_get_temp_size(n, r, max_jobs, CHUNK), dtype=torch.uint8, device=dev)
        fd = ctypes.c_size_t(0)

        def call():
            rc = L.cuda_zstd_seekable_read_ranges(bd._h, st.data_ptr(), size, d_off.data_ptr(), d_len.data_ptr(), d_ptr.data_ptr(), r, max(lens), 0,
                                                  d_st.data_ptr(), ctypes.byref(fd), temp.data_ptr(), temp.numel(), stream)
            assert rc == 0, rc

        return call, out, d_st, fd

    rows = []
    for r, length in ((1, 4096), (64, 4096), (4096, 4096), (65536, 4096), (4096, 256)):
        rng = np.random.default_rng(0x5EEC + r + length)
        offs = [int(v) for v in rng.integers(0, total - length + 1, r)]
        lens = [length] * r
        touched = len({f for o in offs for f in range(o // CHUNK, (o + length - 1) // CHUNK + 1)})
        call, out, d_st, fd = batched(offs, lens, touched)
        t_batched = timed(call)
        assert bool((d_st == 0).all().item()) and fd.value == touched, (fd.value, touched)
        single = torch.zeros(r * length, dtype=torch.uint8, device=dev)

        def loop():
            for k, o in enumerate(offs):
                read(o, length, single.data_ptr() + k * length)

        t_loop = timed(loop)
        assert torch.equal(out, single), "the batched bytes differ from the single reads"
        idx = torch.tensor(offs[:64], dtype=torch.int64, device=dev)[:, None] + torch.arange(length, device=dev)[None, :]
        assert torch.equal(out[: len(offs[:64]) * length].view(-1, length), d_in[idx]), "the bytes differ from the source"
        rows.append({"ranges": r, "length": length, "frames_decoded": fd.value, "batched": t_batched, "loop_of_single_reads": t_loop,
                     "speedup": round(t_loop["ms"] / t_batched["ms"], 2), "batched_us_per_range": round(t_batched["ms"] * 1e3 / r, 3),
                     "loop_us_per_range": round(t_loop["ms"] * 1e3 / r, 3)})
        print(json.dumps(rows[-1]), flush=True)
        del call, out, d_st, single

    # one whole-stream range: the batched call stages every frame, read_all decodes in place
    call, out, d_st, fd = batched([0], [total], n)
    t_whole = timed(call)
    assert int(d_st[0].item()) == 0 and fd.value == n and torch.equal(out, d_in)
    del call, out
    t_read_all = timed(lambda: read(0, total, back.data_ptr()))
    assert torch.equal(back, d_in)
    off = total // 2 + 12345
    t_read_1m = timed(lambda: read(off, 1 << 20, back.data_ptr()))
    assert torch.equal(back[: 1 << 20], d_in[off:off + (1 << 20)])

    res = {
        "workload": f"C3: {n} x 64 KiB mix chunks (seed 0x5EED0003), level 3, with checksums; ranges at seeded random offsets",
        "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "stream_bytes": size,
        "timing": "host clock around each blocking call plus a device synchronise; median, min and max of the steps",
        "workloads": rows,
        "whole_stream": {"batched_one_range": t_whole, "read_all": t_read_all, "ratio": round(t_whole["ms"] / t_read_all["ms"], 3),
                         "frames_decoded": n},
        "single_read_unchanged": {"read_all": t_read_all, "read_1MiB": t_read_1m,
                                  "note": "compare with read_all.ms and read_1MiB.ms of profiles/seekable_bench.json (the parent's run)"},
    }
    if a.resources:
        with open(a.resources) as f:
            res["kernel_resources"] = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

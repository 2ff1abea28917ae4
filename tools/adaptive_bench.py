#!/usr/bin/env python3
"""Cost of adaptive level selection on bench.py's workload (16,384 x 64 KiB mix chunks).

Times, with events on the launch stream and in the same run, alternating over --rounds rounds:
  analyze   cuda_zstd_adaptive_analyze_batch_async over the whole batch (memset of the records,
            the analysis kernel, the finalize kernel), buffers allocated once outside the loop;
  copy      a hipMemcpyAsync device-to-device copy of the same bytes (the floor of any pass
            that reads every byte once is half of this: a copy reads and writes);
  compress  the level-1 nvcomp_zstd_batched_compress_async_v5 step (the fastest parse: what the
            analysis is worth is measured against what it can save or cost there).
Reports each as the median over the rounds, the analysis as a fraction of the other two, and
its read rate.  The statistics of the first chunks are checked against the numpy model
(tests/zh_adaptive_model.py) at this size before anything is timed.  Writes one JSON object to
--out and prints it on one line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "custom-nvcomp-with-zstd_amd"))

CHUNK = 65536
SEED = 0x5EED0003


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sample-bytes", type=int, default=CHUNK)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_analyze.json"))
    a = ap.parse_args()

    import torch

    import cuda_zstd
    import zh_adaptive_model as M
    import zh_testlib as T

    L = cuda_zstd.lib()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    dev = torch.device("cuda:0")
    n = a.chunks
    host = T.gen(T.DG_MIX, n, SEED, CHUNK)
    d_in = torch.from_numpy(host).to(dev)
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    in_ptrs = d_in.data_ptr() + ar * CHUNK
    in_sizes = torch.full((n,), CHUNK, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev)

    levels = torch.empty(n, dtype=torch.int32, device=dev)
    stats = torch.empty(n * ctypes.sizeof(cuda_zstd.AdaptiveStats), dtype=torch.uint8, device=dev)
    a_temp = torch.empty(L.cuda_zstd_adaptive_get_temp_size(n), dtype=torch.uint8, device=dev)

    def analyze():
        rc = L.cuda_zstd_adaptive_analyze_batch_async(in_ptrs.data_ptr(), in_sizes.data_ptr(), n, a.sample_bytes, cuda_zstd.BALANCED,
                                                      stats.data_ptr(), levels.data_ptr(), a_temp.data_ptr(), a_temp.numel(), stream.cuda_stream)
        assert rc == 0, rc

    analyze()
    got = cuda_zstd.adaptive_stats_numpy(stats)
    for i in list(range(8)) + [n - 1]:
        want = M.analyze(host[i * CHUNK:(i + 1) * CHUNK], M.BALANCED, a.sample_bytes)
        assert all(got[i][k] == want[k] for k in ("repeated_pairs", "max_run_length", "pattern_score", "unique_bytes")), i
        assert not want["margin_ok"] or got[i]["level"] == want["level"], i
    level_counts = {int(k): int(v) for k, v in zip(*torch.unique(levels, return_counts=True))}

    bc = cuda_zstd.BatchedCompressor(1, CHUNK)
    slot = (bc.max_out(CHUNK) + 255) // 256 * 256
    slots = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    f_ptrs = slots.data_ptr() + ar * slot
    f_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    f_status = torch.zeros(n, dtype=torch.int32, device=dev)
    c_temp = torch.empty(max(bc.temp_size(n, CHUNK), 256), dtype=torch.uint8, device=dev)
    dst = torch.empty(n * CHUNK, dtype=torch.uint8, device=dev)

    def compress():
        bc.compress_async(in_ptrs, in_sizes, CHUNK, f_ptrs, f_sizes, f_status, c_temp, stream)

    def copy():
        hip.hipMemcpyAsync(dst.data_ptr(), d_in.data_ptr(), n * CHUNK, 3, stream.cuda_stream)

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

    ms = {"analyze": [], "copy": [], "compress": []}
    for _ in range(a.rounds):
        ms["analyze"].append(events(analyze))
        ms["copy"].append(events(copy))
        ms["compress"].append(events(compress))
    assert bool((f_status == 0).all().item())
    med = {k: statistics.median(v) for k, v in ms.items()}
    sampled = n * min(a.sample_bytes, CHUNK)
    res = {
        "workload": f"{n} x {CHUNK} B DG_MIX seed {SEED:#x}, sample_bytes {a.sample_bytes}",
        "device": torch.cuda.get_device_name(dev),
        "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
        "analyze_ms": med["analyze"], "copy_d2d_ms": med["copy"], "compress_level1_ms": med["compress"],
        "rounds_ms": ms,
        "analyze_over_copy": med["analyze"] / med["copy"],
        "analyze_over_compress_level1": med["analyze"] / med["compress"],
        "analyze_read_GBps": sampled / med["analyze"] / 1e6,
        "copy_GBps_each_way": n * CHUNK / med["copy"] / 1e6,
        "compress_level1_GBps": n * CHUNK / med["compress"] / 1e6,
        "levels_balanced": level_counts,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""One stream-ordered call at per-chunk levels against one blocking call per distinct level, on
bench.py's workload (16,384 x 64 KiB mix chunks).

Two level assignments of the same chunks:
  balanced  the levels the BALANCED analysis gives them (cuda_zstd_adaptive_analyze_batch_async);
  uniform   a seeded uniform draw over the selector's eight levels (1, 3, 5, 6, 9, 12, 16, 19).
For each, per round (--rounds rounds, alternating the routes):
  call      device-event time of nvcomp_zstd_batched_compress_levels_async_v5 fed the device level
            array, buffers allocated once outside the loop, after --warmup calls;
  per_level device-event time of one nvcomp_zstd_batched_compress_async_v5 per distinct level over
            that level's chunks, handles, pointer arrays and workspaces made outside the loop: what
            the device spends when the host has already grouped the chunks (no copy, no wait);
  python    wall time of cuda_zstd.compress_batch_levels (the same call plus its allocations, the
            pointer table upload and the one wait for the sizes);
  grouped   wall time of the route compress_batch_adaptive took before that call existed: the
            levels copied to the host, the chunks grouped there, one Manager(level).compress_batch
            per distinct level.
The frames of the first chunks of every class are checked against the grouped route's before
anything is timed.  Reports the medians, every round (the spread), the per-class block counts and
the ratios grouped / call, grouped / python and call / per_level.  --single-level-ab FILE adds
the A/B lines of the single-level benchmark (bench.py's C3 leg on two builds, alternating) recorded
in FILE.  Writes one JSON object to --out and prints it on one line."""
import argparse
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
SELECTOR_LEVELS = [1, 3, 5, 6, 9, 12, 16, 19]
CLASS_NAMES = ["k1_mode2", "k1_mode1", "k1_mode0", "deep_128", "deep_64", "deep_32", "deep_16", "deep_8", "deep_4"]


def parse_class(level):
    if level <= 4:
        return 0 if level <= 1 else 1 if level == 2 else 2
    return 8 if level <= 5 else 7 if level == 6 else 6 if level == 7 else 5 if level <= 9 else 4 if level == 10 else 3


def grouped_route(cuda_zstd, chunks, d_levels, stream=None):
    """compress_batch_adaptive's body before compress_batch_levels (without the analysis)."""
    levels = [int(v) for v in d_levels.cpu()]
    frames = [None] * len(chunks)
    for level in sorted(set(levels)):
        idx = [k for k, v in enumerate(levels) if v == level]
        for k, f in zip(idx, cuda_zstd.Manager(level).compress_batch([chunks[k] for k in idx], stream)):
            frames[k] = f
    return frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--single-level-ab", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_levels.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    import cuda_zstd
    import zh_testlib as T

    dev = torch.device("cuda:0")
    n = a.chunks
    host = T.gen(T.DG_MIX, n, SEED, CHUNK)
    d_in = torch.from_numpy(host).to(dev)
    chunks = [d_in[i * CHUNK:(i + 1) * CHUNK] for i in range(n)]
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    in_ptrs = d_in.data_ptr() + ar * CHUNK
    in_sizes = torch.full((n,), CHUNK, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev)

    balanced, _ = cuda_zstd.analyze_batch_device(in_ptrs, in_sizes, cuda_zstd.BALANCED, CHUNK)
    rng = np.random.default_rng(SEED)
    uniform = torch.from_numpy(rng.choice(SELECTOR_LEVELS, n).astype(np.int32)).to(dev)

    bc = cuda_zstd.BatchedCompressor(3, CHUNK)
    slot = (bc.max_out(CHUNK) + 255) // 256 * 256
    slots = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    f_ptrs = slots.data_ptr() + ar * slot
    f_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    f_status = torch.zeros(n, dtype=torch.int32, device=dev)
    temp = torch.empty(bc.temp_size_levels(n, CHUNK), dtype=torch.uint8, device=dev)

    def events(fn, steps):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / steps

    def wall(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    res = {
        "workload": f"{n} x {CHUNK} B DG_MIX seed {SEED:#x}",
        "device": torch.cuda.get_device_name(dev),
        "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
    }
    for name, d_levels in (("balanced", balanced), ("uniform", uniform)):
        def call():
            bc.compress_levels_async(in_ptrs, in_sizes, d_levels, CHUNK, f_ptrs, f_sizes, f_status, temp, stream)

        lv = d_levels.cpu().numpy()
        classes = np.array([parse_class(int(v)) for v in lv])
        # the first chunks of every class: the call's frames are the grouped route's
        pick = sorted({int(i) for c in set(classes.tolist()) for i in np.flatnonzero(classes == c)[:4]})
        call()
        torch.cuda.synchronize(dev)
        assert bool((f_status == 0).all().item())
        want = grouped_route(cuda_zstd, [chunks[i] for i in pick], d_levels[pick])
        for i, w in zip(pick, want):
            got = slots[i * slot:i * slot + int(f_sizes[i])]
            assert torch.equal(got, w), (name, i, int(lv[i]))
        groups = []
        for level in sorted(set(lv.tolist())):
            idx = torch.from_numpy(np.flatnonzero(lv == level)).to(dev)
            h = cuda_zstd.BatchedCompressor(int(level), CHUNK)
            groups.append((h, in_ptrs[idx].contiguous(), in_sizes[idx].contiguous(), f_ptrs[idx].contiguous(), torch.zeros(len(idx), dtype=torch.int64, device=dev),
                           torch.zeros(len(idx), dtype=torch.int32, device=dev), torch.empty(h.temp_size(len(idx), CHUNK), dtype=torch.uint8, device=dev)))

        def per_level():
            for h, ip, isz, op, osz, ost, tmp in groups:
                h.compress_async(ip, isz, CHUNK, op, osz, ost, tmp, stream)

        ms = {"call": [], "per_level": [], "python": [], "grouped": []}
        for _ in range(a.rounds):
            ms["call"].append(events(call, a.steps))
            ms["per_level"].append(events(per_level, a.steps))
            ms["python"].append(wall(lambda: cuda_zstd.compress_batch_levels(chunks, d_levels)))
            ms["grouped"].append(wall(lambda: grouped_route(cuda_zstd, chunks, d_levels)))
        med = {k: statistics.median(v) for k, v in ms.items()}
        res[name] = {
            "levels": {str(int(k)): int(v) for k, v in zip(*np.unique(lv, return_counts=True))},
            "class_blocks": {CLASS_NAMES[c]: int((classes == c).sum()) for c in range(9)},
            "call_ms": med["call"], "per_level_ms": med["per_level"], "python_ms": med["python"], "grouped_ms": med["grouped"],
            "rounds_ms": ms,
            "spread": {k: (max(v) - min(v)) / statistics.median(v) for k, v in ms.items()},
            "grouped_over_call": med["grouped"] / med["call"],
            "grouped_over_python": med["grouped"] / med["python"],
            "call_over_per_level": med["call"] / med["per_level"],
            "call_GBps": n * CHUNK / med["call"] / 1e6,
            "compressed_bytes": int(f_sizes.sum().item()),
        }
    if a.single_level_ab:
        with open(a.single_level_ab) as f:
            res["single_level_ab"] = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

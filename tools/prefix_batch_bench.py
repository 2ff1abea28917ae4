#!/usr/bin/env python3
"""The per-chunk prefix entries and the many-streams object against the routes they replace.

(a) prefix compress: --chunks x 32 KiB chunks behind 32 KiB prefixes at level 3, once as deltas
    (1 % of the chunk's bytes differ from its prefix) and once unrelated (chunk and prefix from
    different seeds).  Device-event time and ratio of nvcomp_zstd_batched_compress_prefix_async_v5;
    the baseline is nvcomp_zstd_batched_compress_async_v5 over the same chunks without prefixes.
(b) many streams: --streams streams x one 16 KiB chunk per round.  Wall time of one
    StreamBatch.compress_chunks round; the baseline is --streams sequential
    StreamingManager.compress_chunk calls (with history), the route this replaces; and the window
    kernel's own time from HIP events around its launch (cuda_zstd_hip_window_profile).
Every timing is the median of --steps calls after --warmup, with min and max.  --unchanged FILE adds
the A/B record of the paths that must not move (bench.py's legs on two builds, the kernels'
resources) kept in FILE.  Writes one JSON object to --out and prints it on one line."""
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

CHUNK = 32768
STREAM_CHUNK = 16384
SEED = 0x5EED0E00


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=16384)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--unchanged", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefix_batch.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    import cuda_zstd
    import zh_testlib as T

    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)

    def events(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize(dev)
        out = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize(dev)
            out.append(e0.elapsed_time(e1))
        return out

    def wall(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    res = {"device": torch.cuda.get_device_name(dev), "steps": a.steps, "warmup": a.warmup}

    # ---- (a) prefix compress
    n = a.chunks
    rng = np.random.default_rng(SEED)
    pre_host = T.gen(T.DG_MIX, n, SEED, CHUNK)
    delta_host = pre_host.copy()
    changed = rng.integers(0, CHUNK, (n, CHUNK // 100)) + (np.arange(n) * CHUNK)[:, None]
    delta_host[changed.reshape(-1)] ^= rng.integers(1, 256, changed.size, dtype=np.uint8)
    other_host = T.gen(T.DG_MIX, n, SEED + 1, CHUNK)
    d_pre = torch.from_numpy(pre_host).to(dev)
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    sizes = torch.full((n,), CHUNK, dtype=torch.int64, device=dev)
    pre_ptrs = d_pre.data_ptr() + ar * CHUNK
    bc = cuda_zstd.BatchedCompressor(3, CHUNK)
    slot = (bc.max_out(CHUNK) + 255) // 256 * 256
    slots = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    f_ptrs = slots.data_ptr() + ar * slot
    f_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    f_status = torch.zeros(n, dtype=torch.int32, device=dev)
    temp = torch.empty(max(bc.temp_size_prefix(n, CHUNK), bc.temp_size(n, CHUNK)), dtype=torch.uint8, device=dev)
    res["prefix_compress"] = {"workload": f"{n} x {CHUNK} B chunks behind {CHUNK} B prefixes, level 3, DG_MIX seed {SEED:#x}"}
    for name, host in (("delta", delta_host), ("unrelated", other_host)):
        d_in = torch.from_numpy(host).to(dev)
        in_ptrs = d_in.data_ptr() + ar * CHUNK

        def with_prefix():
            bc.compress_prefix_async(in_ptrs, sizes, pre_ptrs, sizes, CHUNK, f_ptrs, f_sizes, f_status, temp, stream)

        def plain():
            bc.compress_async(in_ptrs, sizes, CHUNK, f_ptrs, f_sizes, f_status, temp, stream)

        t_pre = events(with_prefix)
        assert bool((f_status == 0).all().item())
        c_pre = int(f_sizes.sum().item())
        k = n // 2  # one frame against libzstd with the prefix as its dictionary
        frame = slots[k * slot:k * slot + int(f_sizes[k])].cpu().numpy().tobytes()
        assert T.zstd_decompress(frame, CHUNK, dictionary=pre_host[k * CHUNK:(k + 1) * CHUNK].tobytes()) == host[k * CHUNK:(k + 1) * CHUNK].tobytes()
        t_plain = events(plain)
        assert bool((f_status == 0).all().item())
        c_plain = int(f_sizes.sum().item())
        res["prefix_compress"][name] = {
            "prefix": dict(summary(t_pre), ratio=n * CHUNK / c_pre, GBps=n * CHUNK / statistics.median(t_pre) / 1e6),
            "plain": dict(summary(t_plain), ratio=n * CHUNK / c_plain, GBps=n * CHUNK / statistics.median(t_plain) / 1e6),
            "prefix_over_plain_time": statistics.median(t_pre) / statistics.median(t_plain),
        }
        del d_in
    bc.close()
    del slots, temp, d_pre

    # ---- (b) many streams
    ns = a.streams
    rounds = a.warmup + a.steps
    shost = T.gen(T.DG_JSON, ns, SEED + 2, STREAM_CHUNK * rounds)  # stream i: rounds consecutive 16 KiB chunks
    d_s = torch.from_numpy(shost).to(dev)

    def chunk(i, r):
        at = (i * rounds + r) * STREAM_CHUNK
        return d_s[at:at + STREAM_CHUNK]

    sb = cuda_zstd.StreamBatch(3, ns, STREAM_CHUNK)
    L = cuda_zstd.lib()
    t_batch, t_win = [], []
    for r in range(rounds):
        row = [chunk(i, r) for i in range(ns)]
        L.cuda_zstd_hip_window_profile(1, None)
        t = wall(lambda: sb.compress_chunks(row))
        ms = ctypes.c_double()
        L.cuda_zstd_hip_window_profile(0, ctypes.byref(ms))
        if r >= a.warmup:
            t_batch.append(t)
            t_win.append(ms.value)
    sb.close()
    singles = [cuda_zstd.StreamingManager(3) for _ in range(ns)]
    t_seq, seq_bytes = [], 0
    for r in range(rounds):
        def seq():
            return [singles[i].compress_chunk(chunk(i, r), with_history=True) for i in range(ns)]

        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        frames = seq()
        torch.cuda.synchronize(dev)
        if r >= a.warmup:
            t_seq.append((time.perf_counter() - t0) * 1e3)
        seq_bytes = sum(f.numel() for f in frames)
    res["many_streams"] = {
        "workload": f"{ns} streams x {STREAM_CHUNK} B per round, level 3, DG_JSON seed {SEED + 2:#x}, {rounds} rounds ({a.warmup} warm-up)",
        "stream_batch_round": summary(t_batch),
        "sequential_streaming_manager_round": summary(t_seq),
        "window_kernel": summary(t_win),
        "sequential_over_batch": statistics.median(t_seq) / statistics.median(t_batch),
        "last_round_ratio_sequential": ns * STREAM_CHUNK / seq_bytes,
    }
    if a.unchanged:
        with open(a.unchanged) as f:
            res["unchanged_paths"] = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

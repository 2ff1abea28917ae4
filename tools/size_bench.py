#!/usr/bin/env python3
"""The on-device decompressed-size query (nvcomp_zstd_batched_get_decompress_size_async_v5) timed on
bench.py's C3 workload (16,384 x 64 KiB mix chunks, level 3), in one process:

  (1) the query on the C3 frames as the compressor writes them, with a Frame_Content_Size: a walk
      of the frame and block headers;
  (2) the query on the same payloads re-framed without a Frame_Content_Size (the header rewritten
      here as a streaming writer would have written it, the blocks unchanged): every buffer runs
      its sequence bitstream through the length-summing loop;
  (3) the batched decode (nvcomp_zstd_batched_decompress_async_v5, existing code) of the same
      buffers with given capacities, for both framings.

Each figure is the median of --steps calls, every call timed by its own pair of events on the
launch stream, after --warmup calls.  (1) and (2) are reported in milliseconds and as a fraction
of the decode of the same buffers.  Writes one JSON object to --out and prints it on one line.
"""
import argparse
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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "size_bench.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    import cuda_zstd
    import zh_size_model as M
    import zh_testlib as T

    dev = torch.device("cuda:0")
    n = a.chunks
    d_in = torch.from_numpy(T.gen(T.DG_MIX, n, SEED, CHUNK)).to(dev)
    bc, bd = cuda_zstd.BatchedCompressor(3, CHUNK), cuda_zstd.BatchedDecompressor()
    slot = (bc.max_out(CHUNK) + 255) // 256 * 256
    slots = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    in_ptrs, f_ptrs = d_in.data_ptr() + ar * CHUNK, slots.data_ptr() + ar * slot
    in_sizes = torch.full((n,), CHUNK, dtype=torch.int64, device=dev)
    f_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    f_status = torch.zeros(n, dtype=torch.int32, device=dev)
    temp = torch.empty(max(bc.temp_size(n, CHUNK), 256), dtype=torch.uint8, device=dev)
    bc.compress_async(in_ptrs, in_sizes, CHUNK, f_ptrs, f_sizes, f_status, temp)
    torch.cuda.synchronize(dev)
    assert bool((f_status == 0).all().item())
    del temp

    # the same payloads without a Frame_Content_Size: headers rewritten on the host
    host, hsz = slots.cpu().numpy(), f_sizes.cpu().numpy()
    host2, hsz2 = np.zeros_like(host), np.zeros_like(hsz)
    for i in range(n):
        f = M.drop_content_size(host[i * slot:i * slot + int(hsz[i])].tobytes())
        assert f is not None
        host2[i * slot:i * slot + len(f)] = np.frombuffer(f, np.uint8)
        hsz2[i] = len(f)
    slots2, g_sizes = torch.from_numpy(host2).to(dev), torch.from_numpy(hsz2).to(dev)
    g_ptrs = slots2.data_ptr() + ar * slot
    del host, host2

    q_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    q_status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    back = torch.empty(n * CHUNK, dtype=torch.uint8, device=dev)
    back_ptrs = back.data_ptr() + ar * CHUNK
    caps = torch.full((n,), CHUNK, dtype=torch.int64, device=dev)
    d_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    d_status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    dtemp = torch.empty(max(bd.temp_size(n, CHUNK), 256), dtype=torch.uint8, device=dev)

    def median_ms(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize(dev)
        runs = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize(dev)
            runs.append(e0.elapsed_time(e1))
        return statistics.median(runs), [round(r, 4) for r in runs]

    def query(ptrs, sizes):
        q_sizes.zero_()
        q_status.fill_(-1)
        ms = median_ms(lambda: bd.get_sizes_async(ptrs, sizes, q_sizes, q_status))
        assert bool((q_status == 0).all().item()) and bool((q_sizes == CHUNK).all().item())
        return ms

    def decode(ptrs, sizes):
        back.zero_()
        ms = median_ms(lambda: bd.decompress_async(ptrs, sizes, caps, CHUNK, back_ptrs, d_sizes, d_status, dtemp))
        assert bool((d_status == 0).all().item()) and bool((d_sizes == CHUNK).all().item()) and torch.equal(back, d_in)
        return ms

    (q1, q1r), (q2, q2r) = query(f_ptrs, f_sizes), query(g_ptrs, g_sizes)
    (d1, d1r), (d2, d2r) = decode(f_ptrs, f_sizes), decode(g_ptrs, g_sizes)
    r = {
        "workload": f"C3: {n} x 64 KiB mix chunks (seed 0x5EED0003), level 3", "device": torch.cuda.get_device_name(0),
        "timing": f"median of {a.steps} calls after {a.warmup} warm-ups, each call between its own pair of events on the launch stream",
        "compressed_bytes": int(hsz.sum()),
        "query_with_content_size": {"ms": round(q1, 4), "runs_ms": q1r, "fraction_of_decode": round(q1 / d1, 4), "what": "header walk"},
        "query_without_content_size": {"ms": round(q2, 4), "runs_ms": q2r, "fraction_of_decode": round(q2 / d2, 4),
                                       "what": "every buffer's sequence bitstream summed"},
        "decode_with_content_size": {"ms": round(d1, 4), "runs_ms": d1r, "GBps": round(n * CHUNK / (d1 / 1e3) / 1e9, 2)},
        "decode_without_content_size": {"ms": round(d2, 4), "runs_ms": d2r, "GBps": round(n * CHUNK / (d2 / 1e3) / 1e9, 2)},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(r, f, indent=1)
        f.write("\n")
    print(json.dumps(r))


if __name__ == "__main__":
    main()

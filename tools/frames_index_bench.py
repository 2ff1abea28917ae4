#!/usr/bin/env python3
"""The frame index (cuda_zstd_seekable_index) on the C3 stream without its table: 16,384 level-3
frames of 64 KiB mix chunks back to back, and the same frames re-framed without content sizes
(every frame then needs a size job).

Per stream: the auto path (the speculative index) and the forced serial walker of the same build,
the speculative path's per-kernel split by HIP events (candidate write, span, reach, collect; the
hook cuda_zstd_hip_frames_index_split), decompress_frames against read_all of the same frames
packed with their table (the ceiling), and decompress_frames against Manager.decompress of the
buffer as one item (the route it replaces) on a prefix of --one-item-frames frames.  Blocking
calls on the host clock: medians of --steps after --warmup with min and max; a pass over
--long-pass-s seconds is timed once and says so.  --resources: a JSON file of kernel registers,
LDS and scratch in this build and its parent, copied into the result.
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
    ap.add_argument("--one-item-frames", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--long-pass-s", type=float, default=5.0)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_index.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    import cuda_zstd
    import zh_size_model as M
    import zh_testlib as T

    L = cuda_zstd.lib()
    dev = torch.device("cuda:0")
    n = a.chunks
    d_in = torch.from_numpy(T.gen(T.DG_MIX, n, SEED, CHUNK)).to(dev)
    packed = cuda_zstd.seekable_compress(d_in, frame_size=CHUNK, level=3, checksums=False)
    tbytes = 17 + 8 * n
    host = packed.cpu().numpy()
    csizes = host[len(host) - tbytes + 8:len(host) - 9].view("<u4").reshape(-1, 2)[:, 0].astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(csizes)])
    stream = torch.cuda.current_stream(dev).cuda_stream

    def once(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    def timed(fn):
        torch.cuda.synchronize(dev)
        first = once(fn)
        if first > a.long_pass_s * 1e3:
            return {"ms": round(first, 3), "min_ms": round(first, 3), "max_ms": round(first, 3), "steps": 1, "warmup": 0}
        for _ in range(a.warmup - 1):
            fn()
        torch.cuda.synchronize(dev)
        ms = [once(fn) for _ in range(a.steps)]
        return {"ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "steps": a.steps, "warmup": a.warmup}

    def measure(name, frames_host, with_table):
        """frames_host: the frames back to back (numpy); with_table: the same frames packed with a table"""
        size = len(frames_host)
        cap = 17 + 8 * n
        buf = torch.empty(size + cap, dtype=torch.uint8, device=dev)
        buf[:size] = torch.from_numpy(frames_host).to(dev)
        temp = torch.empty(L.cuda_zstd_seekable_index_get_temp_size(size, n), dtype=torch.uint8, device=dev)
        tb, nf, eo = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_ulonglong(0)

        def index():
            rc = L.cuda_zstd_seekable_index(None, buf.data_ptr(), size, n, buf.data_ptr() + size, cap, ctypes.byref(tb), ctypes.byref(nf),
                                            ctypes.byref(eo), temp.data_ptr(), temp.numel(), stream)
            assert rc == 0 and nf.value == n and tb.value == cap, (rc, nf.value, eo.value)

        res = {"stream_bytes": size, "frames": n, "temp_bytes": temp.numel()}
        L.cuda_zstd_hip_frames_index_path(0)
        res["index_auto"] = timed(index)
        assert L.cuda_zstd_hip_frames_index_last_path() == 0
        table_auto = buf[size:].clone()
        L.cuda_zstd_hip_frames_index_path(1)
        res["index_serial"] = timed(index)
        L.cuda_zstd_hip_frames_index_path(0)
        assert torch.equal(table_auto, buf[size:]), "the two paths wrote different tables"
        if with_table is not None:
            assert torch.equal(table_auto, with_table[with_table.numel() - cap:]), "the table differs from the packed stream's"
        res["speculative_over_serial"] = round(res["index_serial"]["ms"] / res["index_auto"]["ms"], 2)
        # per-kernel split of the speculative path (events; the count + sums kernels are the rest of the call)
        split = (ctypes.c_float * 4)()
        L.cuda_zstd_hip_frames_index_split(1, None)
        rows = []
        for _ in range(a.warmup + a.steps):
            index()
            L.cuda_zstd_hip_frames_index_split(1, split)
            rows.append([float(v) for v in split])
        L.cuda_zstd_hip_frames_index_split(0, None)
        rows = rows[a.warmup:]
        res["split_ms"] = {k: {"ms": round(statistics.median(r[i] for r in rows), 4), "min_ms": round(min(r[i] for r in rows), 4),
                               "max_ms": round(max(r[i] for r in rows), 4)} for i, k in enumerate(("write", "span", "reach", "collect"))}
        # end to end: index + read_all against read_all with the table already there
        frames_dev = buf[:size].clone()
        out = []
        res["decompress_frames"] = timed(lambda: out.__setitem__(slice(None), [cuda_zstd.decompress_frames(frames_dev)]))
        assert torch.equal(out[0], d_in), "decompress_frames differs from the source"
        reader = cuda_zstd.SeekableReader(buf[:size + cap])
        res["read_all_with_table"] = timed(lambda: out.__setitem__(slice(None), [reader.read_all()]))
        assert torch.equal(out[0], d_in)
        res["decompress_frames_over_read_all"] = round(res["decompress_frames"]["ms"] / res["read_all_with_table"]["ms"], 3)
        # the route it replaces: the buffer as one item, one workgroup walking the frames
        k = min(a.one_item_frames, n)
        pre = frames_dev[: int(starts_of[name][k])].clone()
        mgr = cuda_zstd.Manager(3)
        res["one_item_prefix"] = {"frames": k, "bytes": pre.numel(),
                                  "manager_decompress": timed(lambda: out.__setitem__(slice(None), [mgr.decompress(pre, capacity=k * CHUNK)])),
                                  "decompress_frames": None}
        assert torch.equal(out[0], d_in[: k * CHUNK]), "Manager.decompress differs from the source"
        res["one_item_prefix"]["decompress_frames"] = timed(lambda: out.__setitem__(slice(None), [cuda_zstd.decompress_frames(pre)]))
        assert torch.equal(out[0], d_in[: k * CHUNK])
        res["one_item_prefix"]["ratio"] = round(res["one_item_prefix"]["manager_decompress"]["ms"] / res["one_item_prefix"]["decompress_frames"]["ms"], 1)
        print(json.dumps({name: res}), flush=True)
        return res

    starts_of = {"with_content_sizes": starts}
    frames = host[: len(host) - tbytes]
    bare = [M.drop_content_size(frames[int(starts[i]):int(starts[i + 1])].tobytes()) for i in range(n)]
    assert all(b is not None for b in bare)
    starts_of["without_content_sizes"] = np.concatenate([[0], np.cumsum([len(b) for b in bare])])
    res = {
        "workload": f"C3: {n} x 64 KiB mix chunks (seed 0x5EED0003), level 3, frames back to back without a table",
        "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
        "timing": "host clock around each blocking call plus a device synchronise; median, min and max of the steps; split_ms by HIP events",
        "with_content_sizes": measure("with_content_sizes", frames, packed),
        "without_content_sizes": measure("without_content_sizes", np.frombuffer(b"".join(bare), np.uint8), None),
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

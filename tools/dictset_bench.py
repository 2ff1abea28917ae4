#!/usr/bin/env python3
"""A batch against a set of dictionaries, against the routes it replaces.

Workload: --records records of 16 KiB JSON (C5's kind) against D in --dicts dictionaries of 64 KiB,
record i against dictionary i mod D, at levels 3 and 9.  The first min(D, --train) dictionaries are
COVER-trained on the device, each on its own 256 records; the others repeat them with the content
rotated by a multiple of 64 bytes (distinct entries with distinct tables, not 1,024 trainings).
Routes, compress and decode (decode over the frames of (a)):
 (a) the set call (nvcomp_zstd_batched_compress_dicts_async_v5 / ..._decompress_dicts_async_v5);
 (b) D = 1 only: the single-dictionary handle over the same chunks -- the ceiling;
 (c) the prefix route with the dictionary contents as prefixes -- what the set replaces;
 (d) the grouped route: one set_dictionary + call per dictionary, in wall time.
(a)-(c) are device time by events, (d) wall time; every timing is the median of --steps calls after
--warmup, with min and max.  Also: creating the set of the largest D against as many set_dictionary
loads.  --unchanged FILE adds the A/B record of the paths that must not move kept in FILE.  Writes
one JSON object to --out and prints it on one line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "custom-nvcomp-with-zstd_amd"))

REC = 16384
DICT = 65536
SEED = 0x5EED0F00


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=16384)
    ap.add_argument("--dicts", type=int, nargs="+", default=[1, 16, 1024])
    ap.add_argument("--train", type=int, default=16)
    ap.add_argument("--levels", type=int, nargs="+", default=[3, 9])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--unchanged", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dictset.json"))
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
        out = []
        for k in range(a.warmup + a.steps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            if k >= a.warmup:
                out.append((time.perf_counter() - t0) * 1e3)
        return out

    n, dmax = a.records, max(a.dicts)
    res = {"device": torch.cuda.get_device_name(dev), "steps": a.steps, "warmup": a.warmup,
           "workload": f"{n} x {REC} B DG_JSON records (seed {SEED:#x}), record i against dictionary i mod D; {min(dmax, a.train)} COVER "
                       f"dictionaries of {DICT} B trained on 256 records each, the others their contents rotated by multiples of 64 B"}
    host = T.gen(T.DG_JSON, n, SEED, REC)
    d_in = torch.from_numpy(host).to(dev)
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    in_ptrs = d_in.data_ptr() + ar * REC
    sizes = torch.full((n,), REC, dtype=torch.int64, device=dev)

    # ---- the dictionaries
    trained = []
    for j in range(min(dmax, a.train)):
        s = torch.from_numpy(T.gen(T.DG_JSON, 256, SEED + 1 + j, REC)).to(dev).view(256, REC)
        trained.append(np.frombuffer(cuda_zstd.Dictionary.train(s, DICT).content(), np.uint8))
    contents = [np.roll(trained[j % len(trained)], 64 * (j // len(trained))).tobytes() for j in range(dmax)]
    assert all(len(c) == DICT for c in contents) and len(set(contents)) == dmax
    handles = [cuda_zstd.Dictionary.load(c) for c in contents]
    d_dicts = torch.from_numpy(np.frombuffer(b"".join(contents), np.uint8).copy()).to(dev)

    # ---- set creation against as many single loads
    loader = cuda_zstd.BatchedCompressor(3, REC)

    def load_all():
        for h in handles:
            loader.set_dictionary(h)

    t_create = wall(lambda: cuda_zstd.DictionarySet(handles).close())
    t_loads = wall(load_all)
    loader.close()
    res["creation"] = {"dictionaries": dmax, "set_create": summary(t_create), "set_dictionary_loads": summary(t_loads),
                       "loads_over_create": statistics.median(t_loads) / statistics.median(t_create)}

    res["compress"], res["decode"] = {}, {}
    for level in a.levels:
        for D in a.dicts:
            key = f"level{level}_D{D}"
            idx = torch.arange(n, dtype=torch.int32, device=dev) % D
            dset = cuda_zstd.DictionarySet(handles[:D])
            bc = cuda_zstd.BatchedCompressor(level, REC)
            slot = (bc.max_out(REC) + 255) // 256 * 256
            slots = torch.empty(n * slot, dtype=torch.uint8, device=dev)
            f_ptrs = slots.data_ptr() + ar * slot
            f_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
            f_status = torch.zeros(n, dtype=torch.int32, device=dev)
            pre_ptrs = d_dicts.data_ptr() + (idx.to(torch.int64)) * DICT
            pre_sizes = torch.full((n,), DICT, dtype=torch.int64, device=dev)
            groups = [(in_ptrs[g::D].contiguous(), sizes[g::D].contiguous(), f_ptrs[g::D].contiguous(), f_sizes[g::D].contiguous(),
                       f_status[g::D].contiguous()) for g in range(D)]
            one = cuda_zstd.BatchedCompressor(level, REC)
            one.set_dictionary(handles[0])
            temp = torch.empty(max(bc.temp_size_dicts(n, REC), one.temp_size(n, REC)), dtype=torch.uint8, device=dev)
            out = {}

            def check(tag):
                assert bool((f_status == 0).all().item()), (key, tag)
                return n * REC / int(f_sizes.sum().item())

            # (c) the prefix route, then (b), then (a) last: its frames stay in the slots for decode
            t = events(lambda: bc.compress_prefix_async(in_ptrs, sizes, pre_ptrs, pre_sizes, REC, f_ptrs, f_sizes, f_status, temp, stream))
            out["c_prefix_route"] = dict(summary(t), ratio=check("c"))
            if D == 1:
                t = events(lambda: one.compress_async(in_ptrs, sizes, REC, f_ptrs, f_sizes, f_status, temp, stream))
                out["b_single_handle"] = dict(summary(t), ratio=check("b"))

            def grouped():
                for g in range(D):
                    one.set_dictionary(handles[g])
                    p, s, fp, fs, st = groups[g]
                    one.compress_async(p, s, REC, fp, fs, st, temp, stream)

            t = wall(grouped)
            out["d_grouped_wall"] = summary(t)
            bc.set_dictionary_set(dset)
            t = events(lambda: bc.compress_dicts_async(in_ptrs, sizes, idx, REC, f_ptrs, f_sizes, f_status, temp, stream))
            out["a_set"] = dict(summary(t), ratio=check("a"), GBps=n * REC / statistics.median(t) / 1e6)
            k = n // 2 + 1  # one frame against libzstd with its dictionary
            frame = slots[k * slot:k * slot + int(f_sizes[k])].cpu().numpy().tobytes()
            assert T.zstd_decompress(frame, REC, dictionary=contents[k % D]) == host[k * REC:(k + 1) * REC].tobytes()
            med = {r: v["median_ms"] for r, v in out.items()}
            out["a_over_c"] = med["a_set"] / med["c_prefix_route"]
            out["a_over_d"] = med["a_set"] / med["d_grouped_wall"]
            if D == 1:
                out["a_over_b"] = med["a_set"] / med["b_single_handle"]
                out["a_inside_b_span"] = out["b_single_handle"]["min_ms"] <= med["a_set"] <= out["b_single_handle"]["max_ms"]
            res["compress"][key] = out

            # ---- decode, over the frames of (a)
            c_sizes = f_sizes.clone()
            outb = torch.empty(n * REC, dtype=torch.uint8, device=dev)
            o_ptrs = outb.data_ptr() + ar * REC
            o_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
            o_status = torch.zeros(n, dtype=torch.int32, device=dev)
            bd = cuda_zstd.BatchedDecompressor()
            dtemp = torch.empty(bd.temp_size(n, REC), dtype=torch.uint8, device=dev)
            dout = {}

            def dcheck(tag):
                assert bool((o_status == 0).all().item()) and bool(torch.equal(outb, d_in)), (key, tag)

            t = events(lambda: bd.decompress_prefix_async(f_ptrs, c_sizes, pre_ptrs, pre_sizes, None, REC, o_ptrs, o_sizes, o_status, dtemp, stream))
            dcheck("c")
            dout["c_prefix_route"] = summary(t)
            dgroups = [(f_ptrs[g::D].contiguous(), c_sizes[g::D].contiguous(), o_ptrs[g::D].contiguous(), o_sizes[g::D].contiguous(),
                        o_status[g::D].contiguous()) for g in range(D)]
            bone = cuda_zstd.BatchedDecompressor()

            def dgrouped():
                for g in range(D):
                    bone.set_dictionary(handles[g])
                    p, s, op, os_, st = dgroups[g]
                    bone.decompress_async(p, s, None, REC, op, os_, st, dtemp, stream)

            if D == 1:
                bone.set_dictionary(handles[0])
                t = events(lambda: bone.decompress_async(f_ptrs, c_sizes, None, REC, o_ptrs, o_sizes, o_status, dtemp, stream))
                dcheck("b")
                dout["b_single_handle"] = summary(t)
            outb.zero_()
            t = wall(dgrouped)
            assert bool(torch.equal(outb, d_in)), (key, "d")
            dout["d_grouped_wall"] = summary(t)
            outb.zero_()
            bd.set_dictionary_set(dset)
            t = events(lambda: bd.decompress_dicts_async(f_ptrs, c_sizes, idx, None, REC, o_ptrs, o_sizes, o_status, dtemp, stream))
            dcheck("a")
            dout["a_set"] = dict(summary(t), GBps=n * REC / statistics.median(t) / 1e6)
            med = {r: v["median_ms"] for r, v in dout.items()}
            dout["a_over_c"] = med["a_set"] / med["c_prefix_route"]
            dout["a_over_d"] = med["a_set"] / med["d_grouped_wall"]
            if D == 1:
                dout["a_over_b"] = med["a_set"] / med["b_single_handle"]
                dout["a_inside_b_span"] = dout["b_single_handle"]["min_ms"] <= med["a_set"] <= dout["b_single_handle"]["max_ms"]
            res["decode"][key] = dout
            print(f"{key}: compress a {out['a_set']['median_ms']:.2f} ms, decode a {dout['a_set']['median_ms']:.2f} ms", file=sys.stderr, flush=True)
            for h in (bc, one, bd, bone):
                h.close()
            dset.close()
            del slots, temp, outb, dtemp

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

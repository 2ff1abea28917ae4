#!/usr/bin/env python3
"""Long-distance matching measured on the C2 shape (one 64 MiB frame) -> profiles/ldm_bench.json.

  repeat : 64 MiB whose second half repeats its first (C2's 16-symbol data): ratio and GB/s with
           matching on and off, libzstd level 3 with long-distance matching at window 27 beside it
  plain  : C2 itself, nothing to find: what the finder costs, on versus off
Every time is the median of 5 calls after a warm-up, one process, HIP events around the whole call
(cuda_zstd_compress with its host sync), around K1 (cuda_zstd_hip_profile_*) and around the finder's
two kernels (cuda_zstd_hip_ldm_profile).  --parent-lib PATH times plain C2 with matching off through
another build of the library (the commit before the feature) and then through this one, the same
way and each in a child process of its own; the spread quoted is that of the five samples themselves.

  min_seg: ZH_LDM_MIN_SEG compared on 2 MiB of the text and JSON corpora followed by a shuffled copy
           of their own 4-16 KiB pieces: frame bytes with this build, and with each
           --min-seg-lib VALUE=PATH (a build of the library with csrc/zh_ldm.h's constant set to
           VALUE, made outside the tree), each in a child process of its own

Not part of bench.py."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "custom-nvcomp-with-zstd_amd"))
C2_BYTES, C2_SEED = 64 << 20, 0x5EED0002
RUNS = 5


def samples_ms(torch, fn, runs=RUNS):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3),
            "samples_ms": [round(x, 3) for x in xs]}


def c2_only(lib_path):
    """cuda_zstd_compress of plain C2 at level 3 through raw ctypes (any build of the library)."""
    import torch

    import zh_testlib as T

    L = ctypes.CDLL(lib_path)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.cuda_zstd_create_manager.restype = vp
    L.cuda_zstd_get_compress_workspace_size.restype = sz
    L.cuda_zstd_get_compress_workspace_size.argtypes = [vp, sz]
    L.cuda_zstd_compress.argtypes = [vp, vp, sz, vp, ctypes.POINTER(sz), vp, sz, vp]
    d = torch.from_numpy(T.gen(T.DG_SYM16, 1, C2_SEED, C2_BYTES)).cuda()
    m = L.cuda_zstd_create_manager(3)
    ws = torch.empty(L.cuda_zstd_get_compress_workspace_size(m, C2_BYTES), dtype=torch.uint8, device="cuda")
    out = torch.empty(C2_BYTES + (C2_BYTES >> 7) + 4096, dtype=torch.uint8, device="cuda")
    size = sz(0)

    def call():
        size.value = out.numel()
        assert L.cuda_zstd_compress(m, d.data_ptr(), C2_BYTES, out.data_ptr(), ctypes.byref(size), ws.data_ptr(), ws.numel(),
                                    torch.cuda.current_stream().cuda_stream) == 0

    r = spread(samples_ms(torch, call))
    r["frame_bytes"] = size.value
    return r


def zstd_long(data, window_log=27):
    """libzstd level 3 with enableLongDistanceMatching (ZSTD_c 160) at that window."""
    import numpy as np

    import zh_testlib as T

    z = T.zstd()
    if z is None:
        return None
    z.ZSTD_createCCtx.restype = ctypes.c_void_p
    z.ZSTD_freeCCtx.argtypes = [ctypes.c_void_p]
    z.ZSTD_CCtx_setParameter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    z.ZSTD_CCtx_setParameter.restype = ctypes.c_size_t
    z.ZSTD_compress2.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    z.ZSTD_compress2.restype = ctypes.c_size_t
    z.ZSTD_compressBound.restype = ctypes.c_size_t
    c = z.ZSTD_createCCtx()
    for p, v in ((100, 3), (101, window_log), (160, 1)):
        assert not z.ZSTD_isError(z.ZSTD_CCtx_setParameter(c, p, v))
    cap = int(z.ZSTD_compressBound(ctypes.c_size_t(len(data))))
    out = np.zeros(cap, np.uint8)
    r = z.ZSTD_compress2(c, out.ctypes.data, cap, data.ctypes.data, len(data))
    z.ZSTD_freeCCtx(c)
    assert not z.ZSTD_isError(r)
    return int(r)


def min_seg_one():
    """Frame bytes of the pieces corpus with the library this process loads (CUDA_ZSTD_HIP_LIB)."""
    import numpy as np
    import torch

    import cuda_zstd
    import zh_testlib as T

    rng = np.random.default_rng(0x5E6)
    base = np.concatenate([T.gen(T.DG_TEXT, 16, 0x5EED0003, 65536), T.gen(T.DG_JSON, 16, 0x5EED0004, 65536)])
    cuts = [0]
    while cuts[-1] < len(base):
        cuts.append(min(len(base), cuts[-1] + int(rng.integers(4096, 16385))))
    pieces = [base[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    data = np.concatenate([base] + [pieces[i] for i in rng.permutation(len(pieces))])
    d = torch.from_numpy(data).cuda()
    m = cuda_zstd.Manager(3, long_distance=27)
    on, off = m.compress(d), cuda_zstd.Manager(3).compress(d)
    torch.cuda.synchronize()
    fb = on.cpu().numpy().tobytes()
    assert T.zstd_decompress(fb, len(data)) == data.tobytes()
    rec = m.ldm_plan(d)
    return {"input_bytes": len(data), "pieces": len(pieces), "frame_bytes": len(fb), "frame_bytes_without_matching": int(off.numel()),
            "cells_split": int((rec[:, 1] > 0).sum()), "bytes_in_one_sequence_blocks": int(rec[:, 1].sum()),
            "shortest_run": int(rec[rec[:, 1] > 0, 1].min()) if (rec[:, 1] > 0).any() else 0}


def leg(torch, cuda_zstd, T, host, on):
    d = torch.from_numpy(host).cuda()
    m = cuda_zstd.Manager(3, long_distance=27 if on else False)
    frame = m.compress(d)
    torch.cuda.synchronize()
    fb = frame.cpu().numpy().tobytes()
    assert T.zstd_decompress(fb, len(host)) == host.tobytes()
    cuda_zstd.profile_enable(True)
    ms = ctypes.c_double(0)
    cuda_zstd.lib().cuda_zstd_hip_ldm_profile(1, None)
    xs = samples_ms(torch, lambda: m.compress(d))
    cuda_zstd.lib().cuda_zstd_hip_ldm_profile(0, ctypes.byref(ms))
    cuda_zstd.profile_enable(False)
    launches, kms = cuda_zstd.profile_collect()
    r = spread(xs)
    r.update({"frame_bytes": len(fb), "ratio": round(len(host) / len(fb), 4), "GBps": round(len(host) / statistics.median(xs) / 1e6, 3),
              "k1_ms_per_call": round(kms[0] / launches, 3), "entropy_ms_per_call": round(kms[1] / launches, 3),
              "ldm_kernels_ms_per_call": round(ms.value / launches, 3), "libzstd_decodes": True})
    if on:
        rec = m.ldm_plan(d)
        r["cells_split"] = int((rec[:, 1] > 0).sum())
        r["workspace_bytes"] = m.workspace_size(len(host))
    m.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c2-only", action="store_true", help="time plain C2 with --lib and print one JSON line")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--parent-lib", default=None, help="a build of the library from the commit before the feature")
    ap.add_argument("--min-seg-one", action="store_true", help="print the pieces corpus result of the loaded library as one JSON line")
    ap.add_argument("--min-seg-lib", action="append", default=[], metavar="VALUE=PATH", help="a build with ZH_LDM_MIN_SEG = VALUE")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldm_bench.json"))
    a = ap.parse_args()
    if a.c2_only:
        print(json.dumps(c2_only(a.lib)))
        return
    if a.min_seg_one:
        print(json.dumps(min_seg_one()))
        return
    import numpy as np
    import torch

    import cuda_zstd
    import zh_testlib as T

    plain = T.gen(T.DG_SYM16, 1, C2_SEED, C2_BYTES)
    repeat = np.concatenate([plain[: C2_BYTES // 2], plain[: C2_BYTES // 2]])
    res = {"device": torch.cuda.get_device_name(0), "method": f"median of {RUNS} calls after a warm-up, HIP events; level 3, window 2^27, table 2^20",
           "repeat": {"workload": "64 MiB, second half = first half, C2's 16-symbol data",
                      "off": leg(torch, cuda_zstd, T, repeat, False), "on": leg(torch, cuda_zstd, T, repeat, True)},
           "plain": {"workload": "C2: 64 MiB iid 16-symbol buffer, nothing to find",
                     "off": leg(torch, cuda_zstd, T, plain, False), "on": leg(torch, cuda_zstd, T, plain, True)}}
    zl = zstd_long(repeat)
    if zl:
        res["repeat"]["libzstd_l3_long27"] = {"frame_bytes": zl, "ratio": round(C2_BYTES / zl, 4)}
    for k in ("repeat", "plain"):
        on = res[k]["on"]
        res[k]["ldm_kernels_below_k1"] = on["ldm_kernels_ms_per_call"] < on["k1_ms_per_call"]
    if a.parent_lib:
        # both builds the same way, each in a process of its own: the other build first
        def child(lib):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--c2-only", "--lib", lib], capture_output=True, text=True, check=True)
            return json.loads(p.stdout.strip().splitlines()[-1])

        parent, off = child(a.parent_lib), child(cuda_zstd.LIB_PATH)
        res["parent_commit_c2"] = parent
        res["this_commit_c2_off"] = off
        res["off_vs_parent"] = {"this_median_ms": off["median_ms"], "parent_median_ms": parent["median_ms"],
                                "this_range_ms": [off["min_ms"], off["max_ms"]], "parent_range_ms": [parent["min_ms"], parent["max_ms"]],
                                "same_frame_bytes": off["frame_bytes"] == parent["frame_bytes"],
                                "ranges_overlap": off["min_ms"] <= parent["max_ms"] and parent["min_ms"] <= off["max_ms"]}
    def seg_child(lib):
        env = dict(os.environ, CUDA_ZSTD_HIP_LIB=lib)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--min-seg-one"], capture_output=True, text=True, check=True, env=env)
        return json.loads(p.stdout.strip().splitlines()[-1])

    res["min_seg"] = {"workload": "2 MiB text + JSON corpora followed by a shuffled copy of their own 4-16 KiB pieces, level 3, window 2^27",
                      "this_build": seg_child(cuda_zstd.LIB_PATH)}
    for spec in a.min_seg_lib:
        v, path = spec.split("=", 1)
        res["min_seg"][f"min_seg_{int(v)}"] = seg_child(os.path.abspath(path))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""COVER training, host against device, on the C5 training sets (tools/c5_dict.py: 4,096 JSON-like
records of 16 KiB, seed 0x5EED0005, 64 KiB dictionary): every fourth record, as
tests/test_gpu_dict.py::test_c5_full_workload_vs_oracle trains it, and all 4,096.

Host: cuda_zstd_train_dictionary over pointers into the host copy of the records.  Device:
Dictionary.train over the device-resident records (rows of one 2-D tensor; every fourth row is
gathered on the device inside the call).  Both are wall time over the whole call in one process,
the device's including its temp allocation, the final synchronisation and the copy of the
dictionary back; a warm-up call first, then the median of 5.  The two dictionaries must be equal
and the device must be the faster one.  The per-kernel split comes from one more device call with
HIP events around the kernel groups (cuda_zstd_hip_dict_train_profile).

Writes profiles/dict_train_device.json and prints it as one JSON line."""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "custom-nvcomp-with-zstd_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import c5_dict as C  # noqa: E402
import cuda_zstd  # noqa: E402
import zh_testlib as T  # noqa: E402

REPS = 5


def median_wall(fn):
    fn()  # warm-up
    ts, out = [], None
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[REPS // 2], ts, out


def host_train(host, rows):
    L = cuda_zstd.lib()
    n = len(rows)
    ptrs = (ctypes.c_void_p * n)(*[host.ctypes.data + r * C.REC for r in rows])
    sizes = (ctypes.c_size_t * n)(*[C.REC] * n)
    return lambda: cuda_zstd.Dictionary(L.cuda_zstd_train_dictionary(ptrs, sizes, n, C.DICT)).content()


def main():
    host = T.gen(T.DG_JSON, C.N, C.SEED, C.REC)
    d_recs = torch.from_numpy(host).cuda().view(C.N, C.REC)
    torch.cuda.synchronize()
    res = {"workload": "COVER training, 64 KiB dictionary, k 1024 / d 8, C5 records (16 KiB JSON-like, seed 0x5EED0005)",
           "device": torch.cuda.get_device_name(0), "timing": f"wall seconds over the whole call, median of {REPS} after a warm-up", "sets": {}}
    ok = True
    for name, step in (("every_4th_record", 4), ("all_records", 1)):
        rows = list(range(0, C.N, step))
        d_set = d_recs[::step]
        t_host, hs, want = median_wall(host_train(host, rows))
        t_dev, ds, got = median_wall(lambda: cuda_zstd.Dictionary.train(d_set, C.DICT).content())
        ms3 = (ctypes.c_double * 3)()
        cuda_zstd.lib().cuda_zstd_hip_dict_train_profile(1, None)
        cuda_zstd.Dictionary.train(d_set, C.DICT)
        cuda_zstd.lib().cuda_zstd_hip_dict_train_profile(0, ms3)
        equal = got == want
        ok = ok and equal and t_dev < t_host
        res["sets"][name] = {
            "records": len(rows), "bytes": len(rows) * C.REC, "dict_bytes": len(want), "equal": equal,
            "host_s": round(t_host, 4), "device_s": round(t_dev, 5), "host_over_device": round(t_host / t_dev, 1),
            "host_runs_s": [round(t, 4) for t in hs], "device_runs_s": [round(t, 5) for t in ds],
            "device_kernel_ms": {"ids_freq": round(ms3[0], 3), "prevdist": round(ms3[1], 3), "step_loop": round(ms3[2], 3)},
        }
    out = os.path.join(ROOT, os.environ.get("DICT_TRAIN_BENCH_OUT", os.path.join("profiles", "dict_train_device.json")))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    assert ok, "device dictionary differs from the host's, or the device trainer is not faster"


if __name__ == "__main__":
    main()

"""One COVER dictionary per group: the grouped device call against a loop of single calls.

Workload: G groups of 64 JSON-like records of 16 KiB (1 MiB per group, seed 0x5EED0D50 + group),
64 KiB dictionaries, k 1024 / d 8; G = 1, 16, 256, 1,024 (the last is 1 GiB of samples, inside the
per-call limit of 2^32 - 64 bytes).

  grouped  cuda_zstd_train_dictionaries_device over all G groups, on this build
  loop     cuda_zstd_train_dictionary_device once per group, on the library named by
           --loop-lib (the build of the parent commit: the route users had before the grouped
           call); without it, on this build

Both are wall seconds over everything a caller pays: the temp query and allocation (torch's
allocator), the call or calls, and reading the dictionaries' bytes back.  Each runs in a worker
process of its own that holds the samples on the device; the driver alternates the two, one
warm-up each, then the median of 5 with min and max.  Every dictionary must be byte-equal between
the two (SHA-256 over all contents in group order).  One more grouped call per G runs with HIP
events around its phases (cuda_zstd_hip_dict_train_profile).  No ratio is required.

Writes profiles/dict_train_set.json (or $DICT_TRAIN_SET_BENCH_OUT) and prints it as one JSON line."""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC, PER_GROUP, DICT, K, D, SEED = 16384, 64, 65536, 1024, 8, 0x5EED0D50
GROUPS = (1, 16, 256, 1024)
REPS = 5


def worker(lib_path, max_groups):
    """Serves 'grouped G', 'loop G', 'phases G' and 'quit' lines on stdin, one JSON line each."""
    import torch  # before the library: both then bind to one HIP runtime

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import zh_testlib as T

    L = ctypes.CDLL(lib_path)
    vp, sz, u = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint
    psz = ctypes.POINTER(sz)

    def fn(name, res, args):
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
        return f

    one_size = fn("cuda_zstd_train_dictionary_device_get_temp_size", sz, [sz, sz, sz, u])
    one = fn("cuda_zstd_train_dictionary_device", ctypes.c_int, [vp, psz, sz, sz, u, u, vp, sz, vp, ctypes.POINTER(vp)])
    content = fn("cuda_zstd_get_dictionary_content", sz, [vp, vp, sz])
    destroy = fn("cuda_zstd_destroy_dictionary", None, [vp])
    profile = fn("cuda_zstd_hip_dict_train_profile", None, [ctypes.c_int, ctypes.POINTER(ctypes.c_double)])
    if hasattr(L, "cuda_zstd_train_dictionaries_device"):
        many_size = fn("cuda_zstd_train_dictionaries_device_get_temp_size", sz, [psz, sz, psz, sz, sz, u])
        many = fn("cuda_zstd_train_dictionaries_device", ctypes.c_int,
                  [vp, psz, sz, psz, sz, sz, u, u, vp, sz, vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int)])

    d_all = torch.empty(max_groups * PER_GROUP * REC, dtype=torch.uint8, device="cuda")
    for g in range(max_groups):
        d_all[g * PER_GROUP * REC:(g + 1) * PER_GROUP * REC] = torch.from_numpy(T.gen(T.DG_JSON, PER_GROUP, SEED + g, REC).reshape(-1))
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    group_bytes = PER_GROUP * REC

    def digest(handles):
        h = hashlib.sha256()
        buf = ctypes.create_string_buffer(DICT)
        sizes = []
        for x in handles:
            n = content(x, buf, DICT)
            h.update(buf.raw[:n])
            sizes.append(n)
            destroy(x)
        return h.hexdigest(), min(sizes), max(sizes)

    def grouped(G):
        sizes = (sz * (G * PER_GROUP))(*[REC] * (G * PER_GROUP))
        counts = (sz * G)(*[PER_GROUP] * G)
        hs = (vp * G)()
        t0 = time.perf_counter()
        need = many_size(sizes, G * PER_GROUP, counts, G, DICT, K)
        temp = torch.empty(need, dtype=torch.uint8, device="cuda")
        rc = many(d_all.data_ptr(), sizes, G * PER_GROUP, counts, G, DICT, K, D, temp.data_ptr(), need, stream, hs, None)
        assert rc == 0 and all(hs), rc
        sha, lo, hi = digest(hs)
        return {"s": time.perf_counter() - t0, "sha": sha, "dict_bytes": [lo, hi], "temp_bytes": need}

    def loop(G):
        sizes = (sz * PER_GROUP)(*[REC] * PER_GROUP)
        hs = []
        t0 = time.perf_counter()
        for g in range(G):
            need = one_size(group_bytes, PER_GROUP, DICT, K)
            temp = torch.empty(need, dtype=torch.uint8, device="cuda")
            h = vp()
            rc = one(d_all.data_ptr() + g * group_bytes, sizes, PER_GROUP, DICT, K, D, temp.data_ptr(), need, stream, ctypes.byref(h))
            assert rc == 0 and h.value, rc
            hs.append(h.value)
        sha, lo, hi = digest(hs)
        return {"s": time.perf_counter() - t0, "sha": sha, "dict_bytes": [lo, hi], "temp_bytes": need}

    def phases(G):
        ms3 = (ctypes.c_double * 3)()
        profile(1, None)
        grouped(G)
        profile(0, ms3)
        return {"ids_freq": round(ms3[0], 3), "prevdist": round(ms3[1], 3), "step_loops": round(ms3[2], 3)}

    print(json.dumps({"ready": torch.cuda.get_device_name(0)}), flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        print(json.dumps({"grouped": grouped, "loop": loop, "phases": phases}[cmd[0]](int(cmd[1]))), flush=True)


class Worker:
    def __init__(self, lib_path, max_groups):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", lib_path, "--max-groups", str(max_groups)],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def ready(self):
        """Waits until the samples lie on the device -> the device's name."""
        return json.loads(self.p.stdout.readline())["ready"]

    def ask(self, what, G):
        self.p.stdin.write(f"{what} {G}\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError(f"the worker ended during '{what} {G}' (exit {self.p.wait()})")
        return json.loads(line)

    def close(self):
        try:
            self.p.stdin.write("quit\n")
            self.p.stdin.flush()
        except OSError:
            pass
        self.p.wait(timeout=60)


def stats(ts):
    return {"median_s": round(sorted(ts)[len(ts) // 2], 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker")
    ap.add_argument("--max-groups", type=int, default=max(GROUPS))
    ap.add_argument("--loop-lib", default=None, help="library for the loop of single calls (the parent commit's build)")
    ap.add_argument("--groups", type=int, nargs="*", default=list(GROUPS))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.max_groups)
    this_lib = os.path.join(ROOT, "custom-nvcomp-with-zstd_amd", "libcuda_zstd_hip.so")
    mg = max(a.groups)
    wg, wl = Worker(this_lib, mg), Worker(a.loop_lib or this_lib, mg)
    res = {"workload": f"G groups of {PER_GROUP} x {REC} B JSON-like records, {DICT} B dictionaries, k {K} / d {D}",
           "device": (wg.ready(), wl.ready())[0],
           "timing": f"wall seconds over temp query + allocation + call(s) + reading the bytes back; the two alternated, median of {REPS} after a warm-up",
           "loop_library": "the parent commit's build" if a.loop_lib else "this build", "groups": {}}
    ok = True
    try:
        for G in a.groups:
            wg.ask("grouped", G), wl.ask("loop", G)  # warm-up
            tg, tl, equal, last = [], [], True, None
            for _ in range(REPS):
                x, y = wg.ask("grouped", G), wl.ask("loop", G)
                tg.append(x["s"]), tl.append(y["s"])
                equal = equal and x["sha"] == y["sha"]
                last = (x, y)
            ok = ok and equal
            sg, sl = stats(tg), stats(tl)
            res["groups"][str(G)] = {"sample_bytes": G * PER_GROUP * REC, "equal": equal, "dict_bytes_min_max": last[0]["dict_bytes"],
                                     "grouped": sg, "loop": sl, "loop_over_grouped": round(sl["median_s"] / sg["median_s"], 2),
                                     "grouped_temp_bytes": last[0]["temp_bytes"], "loop_temp_bytes": last[1]["temp_bytes"],
                                     "grouped_phase_ms": wg.ask("phases", G)}
    finally:
        wg.close(), wl.close()
    out = os.path.join(ROOT, os.environ.get("DICT_TRAIN_SET_BENCH_OUT", os.path.join("profiles", "dict_train_set.json")))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    assert ok, "a dictionary of the grouped call differs from the loop's"


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""CompressionConfig::dict_entropy measured -> profiles/dict_entropy.json.

  records  : JSON-like records (tests' generator, seed 0x5EED0005) of 512 B, 1 KiB, 4 KiB and 16 KiB;
             a 16 KiB ZDICT_trainFromBuffer dictionary trained on the first half, 200 held-out
             records compressed at levels 3 and 9.  Per shape: our ratio with the switch off and on,
             libzstd's ratio (ZSTD_compress_usingDict) with the raw content and with the formatted
             dictionary, and the batch manager's compress throughput with both settings (median of 5
             stream-ordered calls after a warm-up, HIP events).
  finalize : the same content and samples through Dictionary.finalize and through libzstd's
             ZDICT_finalizeDictionary (ctypes): 1 KiB held-out records compressed by libzstd with
             each, and by us (switch on) with each.
  --headline FILE... : bench.py result lines (JSON, one per file; name them parent_* / this_*) are
             folded in as the C3 level 3 headline of the parent commit and of this one.

Not part of bench.py."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "custom-nvcomp-with-zstd_amd"))
SEED, DICT, HELD = 0x5EED0005, 16384, 200


def gpu_batch(torch, cuda_zstd, dev, n, rec, d, level, on):
    """-> (total compressed bytes, GB/s) of n records of rec bytes at dev through the batch manager."""
    bc = cuda_zstd.BatchManager(level, rec, dict_entropy=on)
    bc.set_dictionary(cuda_zstd.Dictionary.load(d))
    slot = (bc.max_out(rec) + 255) // 256 * 256
    out = torch.empty(n * slot, dtype=torch.uint8, device="cuda")
    ar = torch.arange(n, dtype=torch.int64, device="cuda")
    in_ptrs, out_ptrs = dev.data_ptr() + ar * rec, out.data_ptr() + ar * slot
    sizes = torch.full((n,), rec, dtype=torch.int64, device="cuda")
    osz = torch.zeros(n, dtype=torch.int64, device="cuda")
    st = torch.zeros(n, dtype=torch.int32, device="cuda")
    temp = torch.empty(bc.temp_size(n, rec), dtype=torch.uint8, device="cuda")
    run = lambda: bc.compress_async(in_ptrs, sizes, rec, out_ptrs, osz, st, temp)
    run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 1e3)
    assert int((st != 0).sum()) == 0
    return int(osz.sum()), n * rec / statistics.median(ts) / 1e9


def zdict_finalize(T, content, samples, capacity):
    z = T.zstd()
    z.ZDICT_finalizeDictionary.restype = ctypes.c_size_t

    class Params(ctypes.Structure):
        _fields_ = [("compressionLevel", ctypes.c_int), ("notificationLevel", ctypes.c_uint), ("dictID", ctypes.c_uint)]

    z.ZDICT_finalizeDictionary.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                           ctypes.POINTER(ctypes.c_size_t), ctypes.c_uint, Params]
    buf = b"".join(samples)
    sizes = (ctypes.c_size_t * len(samples))(*[len(s) for s in samples])
    out = ctypes.create_string_buffer(capacity)
    r = z.ZDICT_finalizeDictionary(out, capacity, content, len(content), buf, sizes, len(samples), Params(3, 0, 0))
    assert not z.ZDICT_isError(r), "ZDICT_finalizeDictionary failed"
    return out.raw[:r]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dict_entropy.json"))
    ap.add_argument("--headline", nargs="*", default=[])
    a = ap.parse_args()
    import torch

    import cuda_zstd
    import zh_testlib as T

    res = {"workload": f"JSON-like records (seed {SEED:#x}), 16 KiB ZDICT dictionary trained on the first half, {HELD} held-out records",
           "records": [], "finalize": {}}
    for rec in (512, 1024, 4096, 16384):
        n = 2 * max(HELD, (1 << 20) // rec)  # at least 1 MiB of training data
        host = T.gen(T.DG_JSON, n, SEED, rec)
        recs = [host[i * rec:(i + 1) * rec] for i in range(n)]
        d = T.zdict_train(recs[:n // 2], DICT)
        content = d[T.dict_layout(d)[1]:]
        test = recs[n // 2:n // 2 + HELD]
        dev = torch.from_numpy(host[(n // 2) * rec:(n // 2 + HELD) * rec].copy()).cuda()
        total = HELD * rec
        for level in (3, 9):
            off_b, off_gbps = gpu_batch(torch, cuda_zstd, dev, HELD, rec, d, level, False)
            on_b, on_gbps = gpu_batch(torch, cuda_zstd, dev, HELD, rec, d, level, True)
            z_raw = sum(len(T.zstd_compress_dict(r, content, level)) for r in test)
            z_fmt = sum(len(T.zstd_compress_dict(r, d, level)) for r in test)
            row = {"record_bytes": rec, "level": level, "ratio_off": round(total / off_b, 3), "ratio_on": round(total / on_b, 3),
                   "bytes_change_pct": round(100.0 * (on_b - off_b) / off_b, 1), "libzstd_ratio_raw_content": round(total / z_raw, 3),
                   "libzstd_ratio_formatted": round(total / z_fmt, 3), "libzstd_bytes_change_pct": round(100.0 * (z_fmt - z_raw) / z_raw, 1),
                   "compress_GBps_off": round(off_gbps, 3), "compress_GBps_on": round(on_gbps, 3)}
            print(row)
            res["records"].append(row)
        if rec == 1024:
            samples = [r.tobytes() for r in recs[:n // 2]]
            raw = cuda_zstd.Dictionary.load(content)
            ours = raw.finalize(samples).content()
            theirs = zdict_finalize(T, content, samples, len(content) + 4096)
            f = {"content_bytes": len(content), "samples": len(samples), "header_bytes_ours": T.dict_layout(ours)[1],
                 "header_bytes_zdict": T.dict_layout(theirs)[1]}
            for name, dd in (("ours", ours), ("zdict", theirs)):
                f[f"libzstd_l3_ratio_with_{name}"] = round(total / sum(len(T.zstd_compress_dict(r, dd, 3)) for r in test), 3)
                f[f"gpu_l3_ratio_on_with_{name}"] = round(total / gpu_batch(torch, cuda_zstd, dev, HELD, rec, dd, 3, True)[0], 3)
            f["gpu_l3_ratio_raw_content"] = round(total / gpu_batch(torch, cuda_zstd, dev, HELD, rec, content, 3, True)[0], 3)
            print(f)
            res["finalize"] = f
    head = {}
    for path in a.headline:
        with open(path) as fh:
            lines = [json.loads(x) for x in fh if x.strip().startswith("{")]
        if lines:
            head[os.path.splitext(os.path.basename(path))[0]] = lines[-1]
    if head:
        res["headline_c3_level3"] = head
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

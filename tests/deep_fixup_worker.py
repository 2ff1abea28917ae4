"""Run by tests/test_gpu_deep.py::test_forced_fixup_variant in a child process with
CUDA_ZSTD_HIP_LIB pointing at libcuda_zstd_hip_deepfix.so (the deep matcher built with
-DZH_DEEP_FORCE_FIXUP=1): the chain and dictionary inputs through the zh_test_lz_deep hook and a
handful of them as level-9 frames; writes the raw results and the frames to <out>.npz."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "custom-nvcomp-with-zstd_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cuda_zstd  # noqa: E402
import deep_fixup_data as W  # noqa: E402
import test_gpu_deep as G  # noqa: E402


def main():
    out = sys.argv[1]
    cuda_zstd.lib()
    assert os.path.basename(cuda_zstd.LIB_PATH) == W.LIB_NAME, cuda_zstd.LIB_PATH
    res = {}
    cases = W.hook_cases()
    groups = {}
    for k, (nm, pre, blk, tables, depth) in enumerate(cases):
        groups.setdefault((tables, depth), []).append(k)
    for (tables, depth), ks in groups.items():
        got = G.deep_raw([(cases[k][0], cases[k][1], cases[k][2], 0) for k in ks], depth, tables)
        for k, (recs, lits, rle) in zip(ks, got):
            res[f"recs{k}"] = recs
            res[f"lits{k}"] = np.frombuffer(lits, np.uint8)
            res[f"rle{k}"] = np.array([rle], np.int64)
    outs = cuda_zstd.Manager(9).compress_batch([torch.from_numpy(d).cuda() for _, d in W.frame_inputs()])
    torch.cuda.synchronize()
    frames = [o.cpu().numpy().tobytes() for o in outs]
    res["frame_sizes"] = np.array([len(f) for f in frames], np.int64)
    res["frames"] = np.frombuffer(b"".join(frames), np.uint8)
    np.savez(out, **res)


if __name__ == "__main__":
    main()

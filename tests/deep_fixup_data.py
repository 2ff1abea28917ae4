"""Shared workload of the forced fix-up test (tests/test_gpu_deep.py::test_forced_fixup_variant):
the chain inputs and the dictionary inputs of tests/zh_deep_inputs.py for the hook, and a handful of
them as level-9 frames."""
import zh_deep_inputs as D

LIB_NAME = "libcuda_zstd_hip_deepfix.so"
DEPTH = 32


def hook_cases():
    """(name, prefix or content, block, tables, depth)"""
    out = [(nm, pre, blk, 0, DEPTH) for nm, pre, blk, _ in D.cases_periodic() + D.cases_lims()]
    for d in (4, 32):
        out += [(nm, pre, blk, 0, d) for nm, pre, blk, _ in D.cases_decoys(d)]
    for nm, content, blk in D.cases_dict():
        out.append((nm, content, blk, 1, DEPTH))
    return out


def frame_inputs():
    per = {c[0]: c[2] for c in D.cases_periodic()}
    lims = {c[0]: c[2] for c in D.cases_lims()}
    return [(k, per[k]) for k in ("period2_4096", "period5_20000", "period64_20000", "period255_4096")] + \
           [(k, lims[k]) for k in (f"lim{D.HB}", f"lim{2 * D.HB + 1}")] + [("dict_block", D.cases_dict()[0][2])]

"""Adaptive level selection on the host (no GPU needed): cuda_zstd_adaptive_finalize_host -- the
function the finalize kernel runs -- on the integer statistics of the numpy model
(tests/zh_adaptive_model.py) must give the model's derived values, flags and levels.

The inputs reach all five branches of the rule under all three preferences, and all keep the
model's margin from the rule's thresholds (entropy 0.05, compressibility and repetition 0.01),
so every level is compared.  The fp32 derived values are within 2e-4 of the fp64 model: entropy
is a sum of at most 256 non-negative fp32 terms that total at most 8, so a sequential sum is off
by at most 255 * 2^-24 * 8 = 1.2e-4 (the terms' own rounding, a few ulp of 0.53, is far below
that); the other two are exact ratios or 0.075 x the entropy's error."""
import ctypes

import numpy as np
import pytest

import zh_adaptive_model as M

TOL = 2e-4
inputs, NAMES, BRANCH = M.named_inputs, M.NAMES, M.BRANCH


@pytest.fixture(scope="module")
def cz():
    import cuda_zstd

    cuda_zstd.lib()
    return cuda_zstd


def check(cz, data, preference):
    want = M.analyze(data, preference)
    got = cz.adaptive_finalize_host(want["hist"], want["repeated_pairs"], want["max_run_length"], want["pattern_score"], preference)
    for k in ("repeated_pairs", "max_run_length", "pattern_score", "unique_bytes"):
        assert got[k] == want[k], k
    assert got["sample_size"] == want["n"]
    for k in ("entropy", "repetition_ratio", "compressibility"):
        assert abs(got[k] - want[k]) <= TOL, (k, got[k], want[k])
    assert want["margin_ok"]
    assert (got["has_patterns"], got["is_random"]) == (want["has_patterns"], want["is_random"])
    assert got["level"] == want["level"]
    return want


@pytest.mark.parametrize("preference", [M.SPEED, M.BALANCED, M.RATIO])
@pytest.mark.parametrize("name", NAMES)
def test_finalize_matches_model(cz, name, preference):
    want = check(cz, inputs()[name], preference)
    assert want["branch"] == BRANCH.get(name, 4)
    assert want["level"] == M.LEVELS[want["branch"]][preference]


def test_all_branches_reached():
    assert {M.analyze(inputs()[n])["branch"] for n in NAMES} == {0, 1, 2, 3, 4}
    r = M.analyze(inputs()["random_run300"])
    assert r["repetition_ratio"] < 0.1 and r["max_run_length"] == 256  # the second branch through the run alone
    p = M.analyze(inputs()["period50"])
    assert abs(p["compressibility"] - 0.73) < 0.001 and abs(p["repetition_ratio"] - 0.48) < 0.001


@pytest.mark.parametrize("n,score", [(1, 0), (4, 0), (5, 1), (8, 4), (9, 7)])
def test_tiny_zero_buffers(cz, n, score):
    z = np.zeros(n, np.uint8)
    assert M.integer_stats(z)["pattern_score"] == score
    for preference in (M.SPEED, M.BALANCED, M.RATIO):
        check(cz, z, preference)


def test_empty_sample(cz):
    got = cz.adaptive_finalize_host([0] * 256, 0, 0, 0, M.RATIO)
    assert got["level"] == 3 and got["flags"] == 0 and got["sample_size"] == 0
    assert got["entropy"] == 0.0 and got["repetition_ratio"] == 0.0 and got["compressibility"] == 0.0


def test_error_codes(cz):
    L = cz.lib()
    h = (ctypes.c_uint * 256)()
    out = cz.AdaptiveStats()
    assert L.cuda_zstd_adaptive_finalize_host(None, 0, 0, 0, 0, 1, ctypes.byref(out)) == cz.INVALID
    assert L.cuda_zstd_adaptive_finalize_host(h, 0, 0, 0, 0, 1, None) == cz.INVALID
    assert L.cuda_zstd_adaptive_finalize_host(h, 0, 0, 0, 0, 3, ctypes.byref(out)) == cz.INVALID
    assert L.cuda_zstd_adaptive_finalize_host(h, 0, 0, 0, 0, -1, ctypes.byref(out)) == cz.INVALID
    assert L.cuda_zstd_adaptive_finalize_host(h, 0, 0, 0, 0, 2, ctypes.byref(out)) == cz.OK
    # argument checks of the device entries come before any GPU call
    assert L.cuda_zstd_adaptive_get_temp_size(3) == 3 * 259 * 4
    lv = ctypes.c_int()
    assert L.cuda_zstd_adaptive_analyze_batch_async(None, None, 1, 65536, 1, None, ctypes.byref(lv), None, 0, None) == cz.INVALID
    assert L.cuda_zstd_adaptive_analyze_batch_async(None, None, 0, 65536, 5, None, None, None, 0, None) == cz.INVALID
    assert L.cuda_zstd_adaptive_analyze_batch_async(None, None, 0, 0, 1, None, None, None, 0, None) == cz.INVALID
    assert L.cuda_zstd_adaptive_select_level(None, 10, 65536, 1, ctypes.byref(out), None) == cz.INVALID
    assert L.cuda_zstd_adaptive_select_level(ctypes.byref(lv), 0, 65536, 1, ctypes.byref(out), None) == cz.INVALID
    assert L.cuda_zstd_adaptive_select_level(ctypes.byref(lv), 4, 0, 1, ctypes.byref(out), None) == cz.INVALID
    assert L.cuda_zstd_adaptive_select_level(ctypes.byref(lv), 4, 65536, 1, None, None) == cz.INVALID
    assert ctypes.sizeof(cz.AdaptiveStats) == 40 == M.STATS_DTYPE.itemsize

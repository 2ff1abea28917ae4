"""The C++ surface of adaptive level selection (include/cuda_zstd_adaptive.h) through the driver
tests/cpp_adaptive/adaptive.cpp, which uses the reference's call shapes: default and preference
constructors, select_level, set_preference, set_sample_size, enable_quick_analysis,
get_last_characteristics, reset_statistics, the three free functions, and null / zero-size
arguments.  What it prints is checked against the numpy model (tests/zh_adaptive_model.py):
integers exactly, fp32 values within 2e-4 (the bound of tests/test_adaptive_host.py), levels and
flags for inputs that keep the model's margin -- all of these do.  One child process."""
import functools
import os
import subprocess

import numpy as np
import pytest

import zh_adaptive_model as M
import zh_testlib as T

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(T.ROOT, "tests", "cpp_adaptive", "adaptive")
TOL = 2e-4
# CompressionConfig::level_to_strategy
STRATEGY = lambda lv: 0 if lv <= 1 else 1 if lv <= 3 else 2 if lv <= 6 else 3 if lv <= 12 else 4 if lv <= 15 else 5 if lv <= 18 else 6 if lv <= 20 else 7


def lcg_buffer():
    x, out = 12345, np.full(100000, 0x41, np.uint8)
    for i in range(4096):
        x = (1664525 * x + 1013904223) & 0xFFFFFFFF
        out[i] = x >> 24
    return out


@functools.lru_cache(maxsize=None)
def driver_lines():
    assert os.path.exists(DRIVER), "tests/cpp_adaptive/adaptive not built (__graft_entry__.build())"
    r = subprocess.run([DRIVER], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"adaptive: rc {r.returncode}\n{r.stdout}\n{r.stderr}"
    lines = [l.split() for l in r.stdout.splitlines()]
    assert lines[-1] == ["DONE"]
    return {(l[0], l[1]): l[2:] for l in lines[:-1]}


def check_result(tag, data, preference, sample_bytes=65536):
    f = driver_lines()[("R", tag)]
    want = M.analyze(data, preference, sample_bytes)
    assert want["margin_ok"]
    assert int(f[0]) == 0
    assert int(f[1]) == want["level"] and int(f[2]) == STRATEGY(want["level"])
    assert float(f[3]) == 0.85
    for got, k in zip(f[4:7], ("entropy", "repetition_ratio", "compressibility")):
        assert abs(float(got) - want[k]) <= TOL, (k, got, want[k])
    assert int(f[7]) == want["unique_bytes"] and int(f[8]) == want["max_run_length"] and int(f[9]) == 0
    assert (bool(int(f[10])), bool(int(f[11]))) == (want["has_patterns"], want["is_random"])
    assert int(f[12]) > 0  # a reasoning string
    return want


def test_selector_class():
    zeros, lcg = np.zeros(65536, np.uint8), lcg_buffer()
    assert check_result("zeros_default", zeros, M.BALANCED)["level"] == 12
    check_result("lcg_default_stream", lcg, M.BALANCED)
    # set_sample_size(4096): only the generator's bytes count, so the buffer looks random
    assert check_result("lcg_sample4096", lcg, M.BALANCED, 4096)["is_random"]
    assert check_result("zeros_set_ratio", zeros, M.RATIO, 4096)["level"] == 19  # (the sample size set above stays)
    assert check_result("zeros_speed", zeros, M.SPEED)["level"] == 6
    check_result("lcg4096_ratio", lcg[:4096], M.RATIO)
    d = driver_lines()
    assert d[("E", "last_equals_result")] == ["0"] and d[("E", "reset_clears")] == ["0"]
    assert d[("E", "null")] == ["2"] and d[("E", "zero_size")] == ["2"]  # ERROR_INVALID_PARAMETER


def test_free_functions():
    zeros, lcg = np.zeros(65536, np.uint8), lcg_buffer()
    d = driver_lines()
    assert d[("L", "zeros_free_default")] == ["0", str(M.analyze(zeros, M.BALANCED)["level"])]
    assert d[("L", "lcg4096_free_speed")] == ["0", str(M.analyze(lcg[:4096], M.SPEED)["level"])]
    check_result("lcg_free_ratio", lcg, M.RATIO)
    check_result("zeros300_free", zeros[:300], M.BALANCED)
    for tag, data in (("zeros", zeros), ("lcg4096", lcg[:4096])):
        st, comp, ratio = d[("C", tag)]
        want = M.analyze(data)["compressibility"]
        assert abs(want - 0.3) > 0.01
        assert int(st) == 0 and bool(int(comp)) == (want > 0.3) and abs(float(ratio) - (1.0 + 3.0 * want)) <= 3 * TOL
    assert d[("E", "free_null")] == ["2"] and d[("E", "free_zero_size")] == ["2"] and d[("E", "compressible_null")] == ["2"]

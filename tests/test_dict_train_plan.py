"""The device trainer's formulation (csrc/zh_dict_plan.h) against the host trainer, and the
host entry with explicit COVER parameters: no GPU needed.  GPU parity is
tests/test_gpu_dict_train.py."""
import os
import shutil
import subprocess

import pytest

import zh_testlib as T


def test_plan_header_matches_host_trainer_under_sanitizers(tmp_path):
    """tests/cpp/dict_train_check.cpp rebuilds the dictionary serially from the plan header's
    pieces (epoch geometry, [lo, hi] ranges into a difference array, prefix sum, lowest-w arg-max,
    commit rules) and compares it with zh::cover_train over the shape table.  A stand-alone host
    program (its own main) built with ASan + UBSan (runtimes linked into the program)."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "dict_train_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(T.ROOT, "custom-nvcomp-with-zstd_amd", "csrc"), os.path.join(T.ROOT, "tests", "cpp", "dict_train_check.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "dict train plan OK" in r.stdout, r.stdout + r.stderr


def test_params_entry_defaults_equal_plain_entry():
    """cuda_zstd_train_dictionary_params(..., 0, 0) is cuda_zstd_train_dictionary; explicit k / d
    change the result (tests/test_dictionary.py's fixture)."""
    import ctypes

    import cuda_zstd

    a = T.gen(T.DG_JSON, 512, 0x5EED0005, 4096)
    raw = [a[i:i + 4096].tobytes() for i in range(0, len(a), 4096)]
    n = len(raw)
    bufs = [ctypes.create_string_buffer(b, len(b)) for b in raw]
    ptrs = (ctypes.c_void_p * n)(*[ctypes.addressof(b) for b in bufs])
    sizes = (ctypes.c_size_t * n)(*[len(b) for b in raw])
    L = cuda_zstd.lib()
    plain = cuda_zstd.Dictionary(L.cuda_zstd_train_dictionary(ptrs, sizes, n, 16384)).content()
    assert cuda_zstd.Dictionary(L.cuda_zstd_train_dictionary_params(ptrs, sizes, n, 16384, 0, 0)).content() == plain
    assert cuda_zstd.Dictionary(L.cuda_zstd_train_dictionary_params(ptrs, sizes, n, 16384, 1024, 8)).content() == plain
    assert cuda_zstd.Dictionary.train(raw, 16384).content() == plain
    assert cuda_zstd.Dictionary.train(raw, 16384, k=1024, d=8).content() == plain
    other = cuda_zstd.Dictionary.train(raw, 16384, k=256, d=6).content()
    assert 256 <= len(other) <= 16384 and other != plain
    sizes[3] = 0  # the host entries refuse zero-size samples
    assert not L.cuda_zstd_train_dictionary_params(ptrs, sizes, n, 16384, 0, 0)

"""The grouped device trainer's formulation (csrc/zh_dict_plan.h: group records, the look-back
clamped at a group's start, the temp layout's slots and waves) against the host trainer: no GPU
needed.  GPU parity is tests/test_gpu_dict_train_set.py."""
import os
import shutil
import subprocess

import pytest

import zh_testlib as T


def test_grouped_plan_matches_host_trainer_under_sanitizers(tmp_path):
    """tests/cpp/dict_train_set_check.cpp runs a grouped call serially from the plan header's
    pieces and compares every group's dictionary with zh::cover_train on that group alone, over
    the shapes of the GPU tests; it also checks that the slots of a wave do not overlap and that
    the reported temp size covers the layout for every d in [4, 8].  A stand-alone host program
    (its own main) built with ASan + UBSan (runtimes linked into the program)."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "dict_train_set_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(T.ROOT, "custom-nvcomp-with-zstd_amd", "csrc"),
                    os.path.join(T.ROOT, "tests", "cpp", "dict_train_set_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "dict train set plan OK" in r.stdout, r.stdout + r.stderr

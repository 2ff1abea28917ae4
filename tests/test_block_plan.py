"""The block-descriptor rule (csrc/zh_block_plan.h) shared by the host plan and the two device plan
kernels, walked on the host: no GPU needed.  The routes' parity on the GPU is
tests/test_gpu_plan_routes.py."""
import os
import shutil
import subprocess

import zh_testlib as T


def test_block_plan_properties_under_sanitizers(tmp_path):
    """tests/cpp/block_plan_check.cpp walks sizes x levels x dictionaries x history x padding slots
    and asserts that the active blocks tile the frame, the FIRST / LAST / DIRECT flags, the output
    and staging slots, the staged prefixes, the dictionary split below ZH_DEEP_LEVEL and the item
    descriptor.  A stand-alone host program (its own main) built with ASan + UBSan (runtimes linked
    into the program)."""
    cxx = shutil.which("g++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "block_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(T.ROOT, "custom-nvcomp-with-zstd_amd", "csrc"), "-I", os.path.join(T.ROOT, "include"),
                    os.path.join(T.ROOT, "tests", "cpp", "block_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "block plan OK" in r.stdout, r.stdout + r.stderr

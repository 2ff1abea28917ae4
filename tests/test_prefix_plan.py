"""The per-item prefix of the block-descriptor rule (csrc/zh_block_plan.h) and the stream window
arithmetic (csrc/zh_stream_window.h), walked on the host: no GPU needed.  The routes on the GPU are
tests/test_gpu_prefix_batch.py and tests/test_gpu_stream_batch.py."""
import os
import shutil
import subprocess

import zh_testlib as T


def test_prefix_plan_and_window_under_sanitizers(tmp_path):
    """tests/cpp/prefix_plan_check.cpp: an item with a prefix has the descriptors the rule gives a
    batch whose dictionary is that prefix (dict_id 0), an item without one the dictionary-less ones
    plus padding, over sizes x levels x prefix lengths x padding slots; the window function against
    a byte loop over real buffers at every alignment.  A stand-alone host program (its own main)
    built with ASan + UBSan (runtimes linked into the program)."""
    cxx = shutil.which("g++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "prefix_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(T.ROOT, "custom-nvcomp-with-zstd_amd", "csrc"), "-I", os.path.join(T.ROOT, "include"),
                    os.path.join(T.ROOT, "tests", "cpp", "prefix_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "prefix plan OK" in r.stdout, r.stdout + r.stderr

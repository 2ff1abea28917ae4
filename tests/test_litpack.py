"""K1's literal compaction selector (csrc/zh_litpack.h) on the host: no GPU needed."""
import os
import shutil
import subprocess

import pytest


def test_litpack_selector_under_sanitizers(tmp_path):
    """tests/cpp/litpack_check.cpp (its own main) built with ASan + UBSan (runtimes linked into the
    program): all 16 literal masks x byte patterns through the selector and the v_perm_b32 model."""
    cxx = shutil.which("g++")  # (the runtimes are linked statically: gcc's spelling of the flags)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "litpack_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(root, "custom-nvcomp-with-zstd_amd", "csrc"), os.path.join(root, "tests", "cpp", "litpack_check.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "litpack OK" in r.stdout, r.stdout + r.stderr

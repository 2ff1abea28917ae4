"""The arithmetic of the batched range read (csrc/zh_seek_ranges.h) on the CPU: no GPU needed.
The two-level search, the piece -> segment walk and the temp layout run in a stand-alone host
program (tests/cpp/seek_ranges_check.cpp, its own main) against a plain linear loop."""
import os
import shutil
import subprocess

import pytest

import cuda_zstd


def test_ranges_header_under_sanitizers(tmp_path):
    """Built with ASan + UBSan (runtimes linked into the program); every array is exactly as long
    as the table, so a search or a walk that reads past it stops the program."""
    cxx = shutil.which("g++")  # (the runtimes are linked statically: gcc's spelling of the flags)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "seek_ranges_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(root, "custom-nvcomp-with-zstd_amd", "csrc"), os.path.join(root, "tests", "cpp", "seek_ranges_check.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "seek ranges OK" in r.stdout, r.stdout + r.stderr


def test_ranges_temp_size():
    """The size grows with the jobs and the ranges, a job more costs at least its staging slot,
    and jobs beyond the table's entries do not count."""
    f = cuda_zstd.lib().cuda_zstd_seekable_read_ranges_get_temp_size
    assert f(100, 10, 100, 65536) == f(100, 10, 1000, 65536)
    assert f(100, 10, 5, 65536) >= f(100, 10, 4, 65536) + 65536
    assert f(1100, 10, 5, 256) >= f(1100, 10, 4, 256) + 256
    # two u32 per range, each array rounded up to 256 bytes
    assert f(100, 100000, 4, 65536) == f(100, 10, 4, 65536) + 2 * ((400000 + 255) // 256 * 256 - 256)
    assert f(0, 1, 0, 0) > 0

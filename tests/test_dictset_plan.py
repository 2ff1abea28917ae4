"""The dictionary set's host parts (csrc/zh_dictset.h: ID lookup, creation's validation and sort, an
item's entry in the block-descriptor rule), walked on the host: no GPU needed.  The routes on the
GPU are tests/test_gpu_dictset.py and tests/test_dictset_python.py."""
import os
import shutil
import subprocess

import zh_testlib as T


def test_dictset_find_validation_and_plan_under_sanitizers(tmp_path):
    """tests/cpp/dictset_check.cpp: zh_dictset_find against a linear scan over ID arrays of 0 .. 4,096
    entries (first, last, every gap, IDs 0, 1 and 0xFFFFFFFF); creation refuses duplicate non-zero
    IDs and accepts several ID-0 entries; an item with set entry e has the descriptors of a batch
    whose dictionary is that entry's content with its ID, over sizes x levels x content lengths;
    index -1 the dictionary-less ones plus padding; a bad index only inactive slots.  A stand-alone
    host program (its own main) built with ASan + UBSan (runtimes linked into the program)."""
    cxx = shutil.which("g++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "dictset_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(T.ROOT, "custom-nvcomp-with-zstd_amd", "csrc"), "-I", os.path.join(T.ROOT, "include"),
                    os.path.join(T.ROOT, "tests", "cpp", "dictset_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "dictset OK" in r.stdout, r.stdout + r.stderr

"""The host parser of a formatted dictionary's entropy section (csrc/zh_dict_entropy.h), which
builds the encoder's tables at set_dictionary for CompressionConfig::dict_entropy: no GPU needed.
The GPU side is tests/test_gpu_dict_entropy.py."""
import os
import shutil
import subprocess

import pytest

import zh_testlib as T


def test_parser_under_sanitizers(tmp_path):
    """tests/cpp/dict_entropy_check.cpp: a stand-alone host program (its own main) built with
    ASan + UBSan (runtimes linked into the program).  It parses a ZDICT_trainFromBuffer
    dictionary, checks the blob (a complete prefix code, state tables that are permutations,
    costs, repcodes, the content offset the oracle's parser gives), then every truncated copy and
    every single-bit corruption of the entropy section from exactly-sized heap buffers."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    a = T.gen(T.DG_JSON, 512, 0x5EED0005, 4096)
    d = T.zdict_train([a[i:i + 4096] for i in range(0, len(a), 4096)], 16384)
    did, off = T.dict_layout(d)
    assert did >= 32768 and off > 20
    path = tmp_path / "zdict.bin"
    path.write_bytes(d)
    exe = str(tmp_path / "dict_entropy_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(T.ROOT, "custom-nvcomp-with-zstd_amd", "csrc"), os.path.join(T.ROOT, "tests", "cpp", "dict_entropy_check.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe, str(path), str(off)], capture_output=True, text=True)
    assert r.returncode == 0 and "dict entropy parser OK" in r.stdout, r.stdout + r.stderr

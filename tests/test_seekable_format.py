"""Seek-table parsing on the host (cuda_zstd_seekable_info over a host buffer, and the size
helpers): no GPU needed.  The tables are built with `struct`, as in test_gpu_seekable.py."""
import ctypes
import struct

import pytest

import cuda_zstd

CORRUPT = 6


def table(csizes, dsizes, cks=None, n=None, desc=None, magic=0x8F92EAB1, frame_size=None):
    e = 8 if cks is None else 12
    out = struct.pack("<II", 0x184D2A5E, len(csizes) * e + 9 if frame_size is None else frame_size)
    for k in range(len(csizes)):
        out += struct.pack("<II", csizes[k], dsizes[k])
        if cks is not None:
            out += struct.pack("<I", cks[k])
    d = (0x80 if cks is not None else 0) if desc is None else desc
    return out + struct.pack("<IBI", len(csizes) if n is None else n, d, magic)


def info(buf):
    n, tot, mx, ck = ctypes.c_size_t(0), ctypes.c_ulonglong(0), ctypes.c_uint(0), ctypes.c_int(0)
    rc = cuda_zstd.lib().cuda_zstd_seekable_info(buf, len(buf), ctypes.byref(n), ctypes.byref(tot), ctypes.byref(mx), ctypes.byref(ck))
    return rc, n.value, tot.value, mx.value, ck.value


def test_info_on_host_tables():
    cs, ds = [10, 3, 9, 1000], [65536, 0, 1, 12345]
    body = bytes(sum(cs))
    assert info(body + table(cs, ds)) == (0, 4, sum(ds), 65536, 0)
    assert info(body + table(cs, ds, [1, 2, 3, 4])) == (0, 4, sum(ds), 65536, 1)
    assert info(table([], [])) == (0, 0, 0, 0, 0)
    assert len(table([], [])) == 17


@pytest.mark.parametrize("name,kw", [("magic", dict(magic=0x8F92EAB0)), ("reserved bit", dict(desc=0x04)), ("frame size", dict(frame_size=4 * 8 + 8)),
                                     ("n too large", dict(n=0x7FFFFFF)), ("n over the limit", dict(n=0x8000001))])
def test_info_rejects_damaged_tables(name, kw):
    cs, ds = [10, 3, 9, 1000], [65536, 0, 1, 12345]
    assert info(bytes(sum(cs)) + table(cs, ds, **kw))[0] == CORRUPT, name


def test_info_rejects_sums_and_limits():
    cs, ds = [10, 3, 9, 1000], [65536, 0, 1, 12345]
    assert info(bytes(sum(cs) + 1) + table(cs, ds))[0] == CORRUPT
    assert info(bytes(sum(cs)) + table(cs, [0x40000001, 0, 1, 2]))[0] == CORRUPT
    assert info(bytes(sum(cs)) + table(cs, [0x40000000, 0, 1, 2]))[0] == 0
    assert info(b"\x00" * 16)[0] == CORRUPT


def test_size_helpers():
    L = cuda_zstd.lib()
    assert L.cuda_zstd_seekable_max_size(0, 100, 0) == 17
    assert L.cuda_zstd_seekable_max_size(3, 100, 0) == 300 + 3 * 8 + 17
    assert L.cuda_zstd_seekable_max_size(3, 100, 1) == 300 + 3 * 12 + 17
    assert L.cuda_zstd_seekable_pack_get_temp_size(5000) >= 5000 * 8
    full = L.cuda_zstd_seekable_read_get_temp_size(100, 65536)
    assert L.cuda_zstd_seekable_read_get_temp_size_jobs(100, 100, 65536) == full
    assert L.cuda_zstd_seekable_read_get_temp_size_jobs(100, 4, 65536) < full


def test_format_header_under_sanitizers(tmp_path):
    """The encode / parse / validate arithmetic of csrc/zh_seek_format.h in a stand-alone host
    program (its own main) built with ASan + UBSan (runtimes linked into the program); buffers are exactly the table's size."""
    import os
    import shutil
    import subprocess

    cxx = shutil.which("g++")  # (the runtimes are linked statically: gcc's spelling of the flags)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "seek_format_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(root, "custom-nvcomp-with-zstd_amd", "csrc"), os.path.join(root, "tests", "cpp", "seek_format_check.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "seek format OK" in r.stdout, r.stderr

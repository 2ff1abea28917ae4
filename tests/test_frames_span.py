"""zh_frame_span (csrc/zh_frames.h) on the CPU: no GPU needed.  The header's walk runs in a
stand-alone host program (tests/cpp/frames_span_check.cpp, its own main) over the vectors of
zh_frames_model.py, against the frames and verdicts the Python model wrote down for them, and over
every truncation of every frame."""
import os
import shutil
import struct
import subprocess

import pytest

import zh_frames_model as F

NO_FCS = (1 << 64) - 1


def emit(path, vectors):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(vectors)))
        for v in vectors:
            w = F.walk(v)
            f.write(struct.pack("<I", len(v)) + bytes(v) + struct.pack("<I", len(w.frames)))
            for fr in w.frames:
                f.write(struct.pack("<QQQI", fr.off, fr.size, NO_FCS if fr.fcs is None else fr.fcs, int(fr.skippable)))
            f.write(struct.pack("<IQ", w.status, w.err_off))


def test_span_header_under_sanitizers(tmp_path, libzstd):
    """Built with ASan + UBSan (runtimes linked into the program); every buffer is exactly as long
    as the bytes zh_frame_span may read, so a read past the end stops the program."""
    cxx = shutil.which("g++")  # (the runtimes are linked statically: gcc's spelling of the flags)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, data = str(tmp_path / "frames_span_check"), str(tmp_path / "vectors.bin")
    vectors = [s for _, s, _ in F.good_streams()] + [s for _, s in F.malformed_streams()]
    # Window_Log 30 and 31, every Dictionary_ID width, a Frame_Content_Size of 2^64 - 1 (read as absent)
    vectors += [F.header(fcs=4, window_byte=w << 3) + F.raw_block(b"abcd", True) for w in (20, 21)]
    vectors += [F.hand_frame(b"abc", dict_id=d) + F.hand_frame(b"abc", stated=False, dict_id=d) for d in (0x7F, 0x1234, 0x12345678)]
    vectors += [F.header(fcs=NO_FCS, fcs_bytes=8, single=True) + F.raw_block(b"abcd", True) + F.EMPTY]
    emit(data, vectors)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(root, "custom-nvcomp-with-zstd_amd", "csrc"), os.path.join(root, "tests", "cpp", "frames_span_check.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe, data], capture_output=True, text=True)
    assert r.returncode == 0 and "frames span OK: %d vectors" % len(vectors) in r.stdout, r.stdout + r.stderr

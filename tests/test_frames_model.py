"""The frame index's model (zh_frames_model.py) against libzstd on the CPU: no GPU needed.

The model's walk is what csrc/zh_frames.h states and what the GPU tests expect of the device; here
its frame list is the chain of libzstd's ZSTD_findFrameCompressedSize over the same bytes, its
verdict on a malformed stream stops where libzstd's chain stops, and stream + expected table is a
stream libzstd decodes to the content."""
import ctypes

import numpy as np
import pytest

import zh_frames_model as F
import zh_testlib as T

# The decoder rejects a compressed block of 128 KiB or more where it meets the block header;
# ZSTD_findFrameCompressedSize only hops over it (a decode rejects it later).
LIBZSTD_HOPS_OVER = {"compressed_block_128k"}


def chain(z, buf):
    """libzstd's frames of buf: ([(off, size)], offset where the chain broke or None)."""
    z.ZSTD_findFrameCompressedSize.restype = ctypes.c_size_t
    z.ZSTD_findFrameCompressedSize.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    a = np.frombuffer(bytes(buf), np.uint8).copy()
    out, off = [], 0
    while off < len(a):
        r = z.ZSTD_findFrameCompressedSize(a.ctypes.data + off, len(a) - off)
        if z.ZSTD_isError(r):
            return out, off
        out.append((off, int(r)))
        off += int(r)
    return out, None


@pytest.mark.parametrize("name", [n for n, _, _ in F.good_streams()] if T.zstd() else [])
def test_good_vectors(libzstd, name):
    stream, content = next((s, c) for n, s, c in F.good_streams() if n == name)
    w = F.walk(stream)
    want, broke = chain(libzstd, stream)
    assert broke is None and w.status == F.OK
    assert [(f.off, f.size) for f in w.frames] == want
    r = F.index(stream)
    assert r.rc == 0 and r.num_frames == len(want) and len(r.table) == 17 + 8 * len(want)
    ent = np.frombuffer(r.table[8:-9], "<u4").reshape(-1, 2)
    assert [int(c) for c in ent[:, 0]] == [f.size for f in w.frames] and int(ent[:, 0].sum()) == len(stream)
    assert all(int(d) == 0 for f, d in zip(w.frames, ent[:, 1]) if f.skippable)
    assert int(ent[:, 1].sum()) == len(content)
    assert T.zstd_decompress(stream + r.table, len(content)) == content
    # a frame that states no size: its entry is what libzstd decodes it to
    for f, d in zip(w.frames, ent[:, 1]):
        if not f.skippable and f.fcs is None:
            assert len(T.zstd_decompress(stream[f.off:f.off + f.size], int(d) + 1)) == int(d)


@pytest.mark.parametrize("name", [n for n, _ in F.malformed_streams()] if T.zstd() else [])
def test_malformed_vectors(libzstd, name):
    stream = next(s for n, s in F.malformed_streams() if n == name)
    w = F.walk(stream)
    assert w.status != F.OK
    r = F.index(stream)
    assert r.rc == F.CODE[w.status] and r.num_frames == len(w.frames) and r.error_offset == w.err_off and r.table == b""
    # the decoder's own code only for four whole bytes that are no magic, at offset 0
    assert (w.status == F.BAD_MAGIC) == (name == "wrong_first_magic")
    if name in LIBZSTD_HOPS_OVER:
        return
    want, broke = chain(libzstd, stream)
    assert broke == w.err_off and [(f.off, f.size) for f in w.frames] == want


def test_window_limit_is_the_decoders():
    """Window_Log 30 passes and 31 does not (libzstd's 64-bit limit is 31: the decoder's is pinned here)."""
    ok = F.header(fcs=4, window_byte=20 << 3) + F.raw_block(b"abcd", True)
    assert F.walk(ok).status == F.OK
    assert F.walk(F.header(fcs=4, window_byte=21 << 3) + F.raw_block(b"abcd", True)).status == F.CORRUPT


def test_truncations_fail_where_they_are_cut():
    """Every proper prefix of a well-formed stream fails in the frame the cut falls in (or is a
    shorter well-formed stream when the cut is a frame boundary)."""
    stream = F.skippable(b"ab", 3) + T.zstd_compress(F.text(300, 5), checksum=True) + F.EMPTY
    w = F.walk(stream)
    ends = {f.off + f.size for f in w.frames}
    for t in range(1, len(stream)):
        v = F.walk(stream[:t])
        if t in ends:
            assert v.status == F.OK
        else:
            assert v.status == F.CORRUPT and v.err_off == max(f.off for f in w.frames if f.off < t)


def test_temp_size():
    """Monotone in both arguments; 0 for the empty stream the call answers with 2; max_frames
    counts up to the format's limit."""
    import cuda_zstd

    f = cuda_zstd.lib().cuda_zstd_seekable_index_get_temp_size
    assert f(0, 0) == 0 and f(0, 1000) == 0
    sizes, frames = [1, 2, 4095, 4096, 4097, 1 << 20, (1 << 20) + 1, 1 << 27, 1 << 33], [0, 1, 2, 1000, 1001, 1 << 20, F.MAX_FRAMES]
    for s in sizes:
        row = [f(s, n) for n in frames]
        assert row[0] > 0 and row == sorted(row) and len(set(row)) > 3
        assert f(s, F.MAX_FRAMES + 1) == f(s, F.MAX_FRAMES) == f(s, 1 << 40)
    for n in frames:
        col = [f(s, n) for s in sizes]
        assert col == sorted(col) and col[-1] > col[0]
    # one tile count per 4 KiB of stream, and per frame the candidates' arrays and the entries
    assert f(1 << 27, 1000) - f(1 << 20, 1000) >= ((1 << 27) - (1 << 20)) // F.TILE * 4
    assert f(1 << 20, 2000) - f(1 << 20, 1000) >= 1000 * (2 * 8 + 8)

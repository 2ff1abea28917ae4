"""Batched range reads of a seekable stream (cuda_zstd_seekable_read_ranges, zh_seek.hip) on the
MI355X: many ranges given as device arrays, the table scanned once, every touched frame decoded
once, each range's bytes copied to its own destination.

Streams (level 3; builders in zh_seek_cases.py):
  A  37 frames of 4,096 bytes of content (the last partial) from 150,000 bytes, with checksums
  B  1,100 frames of 256 bytes: ranges cross the 1,024-entry tile of the table scan
  C  6 entries assembled by hand: a skippable frame, two frames, an empty frame, a frame, a
     skippable frame -- entries of size 0 first, in the middle and last

Every call writes into a sentinel-filled arena, and every test asserts that no byte outside the
destinations changed.  The anchor is the source: every good range equals its slice."""
import ctypes
import struct

import numpy as np
import pytest

import zh_seek_cases as C
import zh_testlib as T

pytestmark = pytest.mark.gpu

INVALID, CORRUPT, TOO_SMALL, CHECKSUM, SENT = C.INVALID, C.CORRUPT, C.TOO_SMALL, C.CHECKSUM, C.SENT
FS_A = 4096


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def mgr(torch_cuda):
    import cuda_zstd

    return cuda_zstd.Manager(3)


@pytest.fixture(scope="module")
def dec(torch_cuda):
    import cuda_zstd

    return cuda_zstd.BatchedDecompressor()


@pytest.fixture(scope="module")
def stream_a(torch_cuda, mgr):
    chunks = C.split(C.data_a(), FS_A)
    assert len(chunks) == 37 and len(chunks[-1]) == 150000 - 36 * FS_A
    return C.Stream(C.compress_frames(torch_cuda, mgr, chunks), [c.tobytes() for c in chunks], True)


@pytest.fixture(scope="module")
def stream_b(torch_cuda, mgr):
    chunks = C.split(C.data_b(), 256)
    assert len(chunks) == 1100
    return C.Stream(C.compress_frames(torch_cuda, mgr, chunks), [c.tobytes() for c in chunks], False)


@pytest.fixture(scope="module")
def stream_c(torch_cuda, mgr):
    ch = [c.tobytes() for c in C.chunks_c()]
    f = C.compress_frames(torch_cuda, mgr, C.chunks_c())
    return C.Stream([C.skippable(), f[0], f[1], C.EMPTY_FRAME, f[2], C.skippable(b"tail!")], [b"", ch[0], ch[1], b"", ch[2], b""], True)


def ranges_a(total=150000):
    """One range of each kind of the issue's list (case 1)."""
    return [(70000, 0),  # empty in the middle
            (total, 0),  # empty at offset == total
            (0, 1), (total - 1, 1),  # the first and the last byte
            (5 * FS_A + 100, 1000),  # inside one frame
            (7 * FS_A, FS_A),  # exactly one frame
            (11 * FS_A - 5, 10),  # straddling two frames
            (14 * FS_A + 33, 4 * FS_A - 33 + 7),  # five frames (14..18), both edges partial
            (0, total),  # the whole stream
            (20 * FS_A + 9, 5000), (20 * FS_A + 9, 5000),  # the same range twice
            (25 * FS_A + 1, 6000), (26 * FS_A - 100, 6000),  # two overlapping ranges
            (34 * FS_A, 777), (31 * FS_A + 5, 4100), (29 * FS_A - 1, 2)]  # descending offsets


@pytest.fixture(scope="module")
def ranges_b(stream_b):
    """Case 3's ranges: three across the tile edge, then 300 seeded ones of 1..700 bytes."""
    rng = np.random.default_rng(1100)
    out = [(1023 * 256 - 3, 262), (1024 * 256, 256), (1000 * 256 + 1, 40 * 256)]
    for _ in range(300):
        n = int(rng.integers(1, 701))
        out.append((int(rng.integers(0, stream_b.total - n + 1)), n))
    return out


@pytest.fixture(scope="module")
def result_b(torch_cuda, dec, stream_b, ranges_b):
    """One batched read of case 3's ranges, shared by cases 3 and 7 (max_length: the longest)."""
    ml = max(n for _, n in ranges_b)
    assert ml == 40 * 256
    return C.read_ranges(torch_cuda, dec, stream_b.bytes, stream_b.info, ranges_b, max_length=ml)


# ---- 1: one range of each kind -----------------------------------------------------------------
@pytest.mark.parametrize("verify", [0, 1])
def test_every_kind_of_range(torch_cuda, dec, stream_a, verify):
    s, r = stream_a, ranges_a()
    assert s.total == 150000 and len(s.touched([r[7]])) == 5
    res = C.read_ranges(torch_cuda, dec, s.bytes, s.info, r, verify=verify)
    C.check(res, s, r)
    assert res.frames_decoded == 37  # (the whole-stream range touches them all)
    sub = [q for q in r if q[1] != s.total]
    res = C.read_ranges(torch_cuda, dec, s.bytes, s.info, sub, verify=verify)
    C.check(res, s, sub)
    want = len(s.touched(sub))
    assert 10 < want < 37 and res.frames_decoded == want  # frames under several ranges count once


# ---- 2: destination alignment ------------------------------------------------------------------
def test_destination_alignment(torch_cuda, dec, stream_a):
    """16 ranges of 100 bytes from one frame at source offsets k, into destinations at
    base + 128 k + (15 - k): every destination alignment mod 16 against every source offset.
    (A stride of 64 would lay the 100-byte destinations over each other; 128 k keeps the same
    alignments, 128 k = 64 k = 0 mod 16, with the destinations apart.)"""
    s = stream_a
    f = 3 * FS_A + 40
    r = [(f + k, 100) for k in range(16)]
    dst = [256 + 128 * k + (15 - k) for k in range(16)]
    res = C.read_ranges(torch_cuda, dec, s.bytes, s.info, r, dst_offsets=dst, arena_bytes=256 + 128 * 16 + 256)
    C.check(res, s, r)
    assert res.frames_decoded == 1


# ---- 3: ranges across the scan's tile edge -----------------------------------------------------
def test_ranges_cross_the_tile(stream_b, ranges_b, result_b):
    C.check(result_b, stream_b, ranges_b)
    assert result_b.frames_decoded == len(stream_b.touched(ranges_b))


# ---- 4: entries of size 0 ----------------------------------------------------------------------
def test_zero_size_entries(torch_cuda, dec, stream_c):
    s = stream_c
    assert s.ds == [0, 3000, 4097, 0, 511, 0] and s.starts == [0, 0, 3000, 7097, 7097, 7608]
    r = [(0, 1), (0, 3000), (0, 3001), (2999, 2), (3000, 4097), (7096, 1), (7096, 2), (7097, 1), (7097, 511), (7000, 608), (7607, 1), (7608, 0),
         (7097, 0), (0, 0), (0, 7608)]
    res = C.read_ranges(torch_cuda, dec, s.bytes, s.info, r, verify=1)
    C.check(res, s, r)
    assert res.frames_decoded == 3  # no job for an entry of size 0
    for sub, want in (([(7096, 2)], 2), ([(7097, 0), (0, 0), (7608, 0)], 0), ([(7097, 511)], 1), ([(0, 1)], 1)):
        res = C.read_ranges(torch_cuda, dec, s.bytes, s.info, sub)
        C.check(res, s, sub)
        assert res.frames_decoded == want, sub


# ---- 5: a failure that belongs to one range ----------------------------------------------------
def test_invalid_ranges(torch_cuda, dec, stream_a):
    s = stream_a
    r = ranges_a()[2:8] + [(s.total - 9, 10), (1000, 4 * FS_A + 1), (s.total + 1, 0)]
    ml = 4 * FS_A
    res = C.read_ranges(torch_cuda, dec, s.bytes, s.info, r, max_length=ml)
    C.check(res, s, r, failed={6: INVALID, 7: INVALID, 8: INVALID})  # offset + length == total + 1; length == max_length + 1; offset past the end
    assert res.frames_decoded == len(s.touched(r, ml))


def test_checksum_mismatch_fails_its_ranges(torch_cuda, dec, stream_a):
    s = stream_a
    bad = s.patched(s.table_at + 8 + 12 * 9 + 8, "<I", s.cks[9] ^ 0x10)
    r = ranges_a()
    on9 = {k: CHECKSUM for k, q in enumerate(r) if 9 in s.touched([q])}
    assert len(on9) == 1 and r[8] == (0, s.total)  # (only the whole stream lies over frame 9: add ranges on it)
    r += [(9 * FS_A, 1), (10 * FS_A - 1, 2), (8 * FS_A + 5, 3 * FS_A), (9 * FS_A + 7, 100)]
    on9 = {k: CHECKSUM for k, q in enumerate(r) if 9 in s.touched([q])}
    assert len(on9) == 5
    res = C.read_ranges(torch_cuda, dec, bad, s.info, r, verify=1)
    C.check(res, s, r, failed=on9)
    res = C.read_ranges(torch_cuda, dec, bad, s.info, r, verify=0)
    C.check(res, s, r)


def _corruptions(frame):
    """Candidates for one damaged byte of a frame's body: the first block's type made the
    reserved one, the byte behind the block header, a byte in the middle."""
    fhd = frame[4]
    fcs = {0: 1 if fhd & 0x20 else 0, 1: 2, 2: 4, 3: 8}[fhd >> 6]
    bh = 4 + 1 + (0 if fhd & 0x20 else 1) + (0, 1, 2, 4)[fhd & 3] + fcs
    return [(bh, frame[bh] | 0x06), (bh + 3, frame[bh + 3] ^ 0xFF), (len(frame) // 2, frame[len(frame) // 2] ^ 0xFF)]


def test_undecodable_frame_fails_its_ranges(torch_cuda, dec, mgr, stream_a):
    s = stream_a
    tries = []
    for pos, v in _corruptions(s.frames[20]):
        b = bytearray(s.frames[20])
        b[pos] = v
        tries.append((pos, v, bytes(b)))
    _, codes = mgr.decompress_batch([C.dev(torch_cuda, t[2]) for t in tries], capacities=[FS_A] * len(tries), raise_on_error=False)
    rejected = [(t, c) for t, c in zip(tries, codes) if c != 0]
    assert rejected, "the decoder accepted every damaged frame"
    (pos, v, _), code = rejected[0]
    bad = s.patched(s.cstarts[20] + pos, "<B", v)
    r = ranges_a() + [(20 * FS_A + 4095, 1), (19 * FS_A + 4095, 2), (21 * FS_A, 1)]
    on20 = {k: code & 0xFF for k, q in enumerate(r) if 20 in s.touched([q])}
    assert len(on20) == 5
    res = C.read_ranges(torch_cuda, dec, bad, s.info, r)
    C.check(res, s, r, failed=on20)
    # two failing frames under one range: the lower frame's code (9: checksum, 20: the decoder's)
    b2 = bytearray(bad)
    struct.pack_into("<I", b2, s.table_at + 8 + 12 * 9 + 8, s.cks[9] ^ 1)
    r2 = [(0, s.total), (10 * FS_A, 11 * FS_A), (9 * FS_A + 1, 2), (21 * FS_A, 5)]
    res = C.read_ranges(torch_cuda, dec, bytes(b2), s.info, r2, verify=1)
    C.check(res, s, r2, failed={0: CHECKSUM, 1: code & 0xFF, 2: CHECKSUM})


# ---- 6: a failure of the whole call ------------------------------------------------------------
def _untouched(res, r):
    return res.clean and res.statuses == [C.STATUS_SENT] * len(r) and all(g == bytes([SENT]) * len(g) for g in res.got)


def test_damaged_table_fails_the_call(torch_cuda, dec, stream_a):
    s, r = stream_a, ranges_a()
    n = len(s.ds)
    cases = {
        "seekable magic": s.patched(len(s.bytes) - 4, "<I", 0x8F92EAB0),
        "reserved bit": s.patched(len(s.bytes) - 5, "<B", 0x80 | 0x10),
        "frame size": s.patched(s.table_at + 4, "<I", n * 12 + 9 + 12),
        "csize sum": s.patched(s.table_at + 8, "<I", s.cs[0] + 1),
        "n too large": s.patched(len(s.bytes) - 9, "<I", 0x7FFFFFF),
    }
    for name, b in cases.items():
        res = C.read_ranges(torch_cuda, dec, b, s.info, r, verify=1)
        assert res.rc == CORRUPT, name
        assert _untouched(res, r) and res.frames_decoded == 0, name


def test_short_temp_fails_the_call(torch_cuda, dec, stream_a, stream_b):
    for s, r in ((stream_a, [q for q in ranges_a() if q[1] != stream_a.total]), (stream_b, [(1000 * 256 + 1, 40 * 256), (5, 300)])):
        touched = len(s.touched(r))
        res = C.read_ranges(torch_cuda, dec, s.bytes, s.info, r, max_jobs=touched)  # exactly enough
        C.check(res, s, r)
        assert res.frames_decoded == touched
        res = C.read_ranges(torch_cuda, dec, s.bytes, s.info, r, max_jobs=touched, temp_delta=-1)
        assert res.rc == TOO_SMALL and _untouched(res, r)
        res = C.read_ranges(torch_cuda, dec, s.bytes, s.info, r, max_jobs=touched - 1)
        assert res.rc == TOO_SMALL and _untouched(res, r)
    import cuda_zstd

    need = cuda_zstd.lib().cuda_zstd_seekable_read_ranges_get_temp_size(stream_a.info[0], 1, 0, stream_a.info[1])
    res = C.read_ranges(torch_cuda, dec, stream_a.bytes, stream_a.info, [(0, 10)], max_jobs=0, temp_delta=16 - need)
    assert res.rc == TOO_SMALL and _untouched(res, [(0, 10)])  # below the part sized by the table: nothing is launched


def test_no_ranges(torch_cuda, dec, stream_a):
    res = C.read_ranges(torch_cuda, dec, stream_a.bytes, stream_a.info, [])
    assert res.rc == 0 and res.clean and res.frames_decoded == 0


# ---- 7: the same bytes as the single read ------------------------------------------------------
def test_equals_single_reads(torch_cuda, dec, stream_b, ranges_b, result_b):
    import cuda_zstd

    L = cuda_zstd.lib()
    s = stream_b
    d = C.dev(torch_cuda, s.bytes)
    need = L.cuda_zstd_seekable_read_get_temp_size(*s.info)
    temp = torch_cuda.empty(need, dtype=torch_cuda.uint8, device="cuda")
    ml = max(n for _, n in ranges_b)
    out = torch_cuda.zeros(len(ranges_b) * ml, dtype=torch_cuda.uint8, device="cuda")
    written = ctypes.c_size_t(0)
    for k, (off, n) in enumerate(ranges_b):
        rc = L.cuda_zstd_seekable_read(dec._h, d.data_ptr(), len(s.bytes), off, n, out.data_ptr() + k * ml, ctypes.byref(written), 0, temp.data_ptr(),
                                       need, torch_cuda.cuda.current_stream().cuda_stream)
        assert (rc, written.value) == (0, n), (k, off, n)
    single = out.cpu().numpy()
    for k, (off, n) in enumerate(ranges_b):
        assert result_b.got[k] == single[k * ml:k * ml + n].tobytes(), (k, off, n)


# ---- 8: the Python reader ----------------------------------------------------------------------
def test_python_read_ranges(torch_cuda, stream_a):
    import cuda_zstd

    torch = torch_cuda
    s, r = stream_a, ranges_a()
    offs, lens = [o for o, _ in r], [n for _, n in r]
    side = torch.cuda.Stream()
    d = C.dev(torch, s.bytes)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):  # the offsets are produced on the side stream, and nothing waits before the call
        d_off = torch.tensor(offs, dtype=torch.int64).pin_memory().to("cuda", non_blocking=True) + 0
        d_len = torch.tensor(lens, dtype=torch.int64).pin_memory().to("cuda", non_blocking=True) + 0
    reader = cuda_zstd.SeekableReader(d)
    views = reader.read_ranges(d_off, d_len, verify=True, stream=side)
    assert [v.cpu().numpy().tobytes() for v in views] == [s.data[o:o + n] for o, n in r]
    assert views[3].data_ptr() == views[2].data_ptr() + lens[2] and views[8].data_ptr() == views[2].data_ptr() + sum(lens[2:8])  # one packed buffer
    host = cuda_zstd.SeekableReader(s.bytes).read_ranges(offs, lens)
    assert host == [s.data[o:o + n] for o, n in r]
    assert reader.read_ranges([], []) == []
    # a failing range
    r2 = r[2:6] + [(s.total - 1, 2)]
    with pytest.raises(cuda_zstd.ZstdError) as e:
        reader.read_ranges([o for o, _ in r2], [n for _, n in r2])
    assert e.value.code == INVALID
    views, st = reader.read_ranges([o for o, _ in r2], [n for _, n in r2], raise_on_error=False)
    assert [int(v) for v in st] == [0, 0, 0, 0, INVALID]
    assert [v.cpu().numpy().tobytes() for v in views[:4]] == [s.data[o:o + n] for o, n in r2[:4]]
    bad = cuda_zstd.SeekableReader(C.dev(torch, s.patched(s.table_at + 8 + 12 * 9 + 8, "<I", s.cks[9] ^ 2)))
    _, st = bad.read_ranges([0, 9 * FS_A + 1, 10 * FS_A], [10, 10, 10], verify=True, raise_on_error=False)
    assert [int(v) for v in st] == [0, CHECKSUM, 0]


# ---- 9: frames written with a dictionary -------------------------------------------------------
def test_ranges_with_a_dictionary(torch_cuda, stream_a):
    import cuda_zstd

    s0 = stream_a
    raw = T.gen(T.DG_TEXT, 1, 0xA11CE, 65536)[1000:1000 + 16384].tobytes()  # content the stream's first frames repeat
    m = cuda_zstd.Manager(3)
    m.set_dictionary(cuda_zstd.Dictionary.load(raw))
    s = C.Stream(C.compress_frames(torch_cuda, m, C.split(C.data_a(), FS_A)), s0.contents, True)
    assert sum(s.cs) < sum(s0.cs), "the dictionary changed nothing: the frames would decode without it"
    bd = cuda_zstd.BatchedDecompressor()
    bd.set_dictionary(cuda_zstd.Dictionary.load(raw))
    r = ranges_a()
    res = C.read_ranges(torch_cuda, bd, s.bytes, s.info, r, verify=1)
    C.check(res, s, r)
    assert res.frames_decoded == 37
    views = cuda_zstd.SeekableReader(C.dev(torch_cuda, s.bytes), manager=bd).read_ranges([o for o, _ in r], [n for _, n in r], verify=True)
    assert [v.cpu().numpy().tobytes() for v in views] == [s.data[o:o + n] for o, n in r]

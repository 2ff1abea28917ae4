"""Seekable Zstandard streams (zh_seek.hip): device packing and range reads on the MI355X.

The expected seek tables are built here with `struct` and the oracle's XXH64, a restatement of
the format that shares no code with the library:

    u32 0x184D2A5E | u32 N*E + 9 | N x { u32 csize; u32 dsize; [u32 xxh64 low 32] } | u32 N |
    u8 descriptor (bit 7: checksums) | u32 0x8F92EAB1          (little-endian; E = 8 or 12)

Anchors: the packed stream equals the joined frames of Manager.compress_batch plus that table,
stock libzstd decodes it whole, and every range read equals the input's slice."""
import ctypes
import struct

import numpy as np
import pytest

import zh_testlib as T

pytestmark = pytest.mark.gpu

INVALID, CORRUPT, TOO_SMALL, CHECKSUM = 2, 6, 7, 10
SENT = 0xA5
PAD = 64


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


def xxh32lo(b):
    a = np.frombuffer(bytes(b), np.uint8).copy() if len(b) else np.zeros(1, np.uint8)
    return int(T.oracle().orc_xxh64(a.ctypes.data, len(b))) & 0xFFFFFFFF


def table(csizes, dsizes, cks=None):
    n, e = len(csizes), 8 if cks is None else 12
    out = struct.pack("<II", 0x184D2A5E, n * e + 9)
    for k in range(n):
        out += struct.pack("<II", csizes[k], dsizes[k])
        if cks is not None:
            out += struct.pack("<I", cks[k])
    return out + struct.pack("<IBI", n, 0x80 if cks is not None else 0, 0x8F92EAB1)


def _dev(torch, b):
    a = np.frombuffer(bytes(b), np.uint8).copy()
    return torch.from_numpy(a if a.size else np.zeros(1, np.uint8)).cuda()[: len(b)]


def _pack(torch, chunks, checksums, stream=None, cap_delta=None, bad_status=None, sync_between=True):
    """compress_async + pack_seekable_async over device arrays; returns (whole out buffer as
    bytes, out_size, status, capacity).  cap_delta: capacity = exact stream size + cap_delta
    (needs a first run to learn it: pass the size as a tuple (size, delta))."""
    import cuda_zstd

    n = len(chunks)
    comp = cuda_zstd.BatchedCompressor(3, 65536)
    slot = (comp.max_out(65536) + 255) // 256 * 256
    s = stream if stream is not None else torch.cuda.current_stream()
    ins = [_dev(torch, c.tobytes()) for c in chunks]
    cap = cuda_zstd.BatchedCompressor.seekable_max_size(n, slot, checksums) + PAD if cap_delta is None else cap_delta[0] + cap_delta[1]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        in_ptrs = torch.tensor([t.data_ptr() for t in ins], dtype=torch.int64).cuda()
        in_sizes = torch.tensor([len(c) for c in chunks], dtype=torch.int64).cuda()
        slots = torch.empty(max(n * slot, 1), dtype=torch.uint8, device="cuda")
        f_ptrs = torch.tensor([slots.data_ptr() + k * slot for k in range(n)], dtype=torch.int64).cuda()
        f_sizes = torch.zeros(n, dtype=torch.int64, device="cuda")
        f_status = torch.zeros(n, dtype=torch.int32, device="cuda")
        temp = torch.empty(max(comp.temp_size(n, 65536), comp.pack_temp_size(n), 256), dtype=torch.uint8, device="cuda")
        out = torch.full((cap + PAD,), SENT, dtype=torch.uint8, device="cuda")
        d_size = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        d_status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        if n:
            comp.compress_async(in_ptrs, in_sizes, 65536, f_ptrs, f_sizes, f_status, temp, s)
        if bad_status is not None:  # (the only case that touches the arrays between the two calls)
            f_status[bad_status[0]] = bad_status[1]
        if sync_between:
            torch.cuda.synchronize()
        # `out` is handed over as cap bytes: the PAD bytes behind it must keep the sentinel too
        comp.pack_seekable_async(f_ptrs, f_sizes, f_status, in_ptrs, in_sizes, slot, out[:cap], d_size, d_status, temp, checksums, s)
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes(), int(d_size.item()), int(d_status.item()), cap


def _chunks1():
    rng = np.random.default_rng(77)
    return [T.gen(T.DG_TEXT, 1, 21, 65536), T.gen(T.DG_MIX, 1, 22, 65536), np.array([0x42], np.uint8), T.gen(T.DG_TEXT, 1, 23, 12345),
            T.gen(T.DG_MIX, 1, 24, 65535), rng.integers(0, 256, 40000, dtype=np.uint8), np.zeros(65536, np.uint8)]


class Case:
    """Chunks, their frames (Manager.compress_batch) and the expected streams, computed once."""

    def __init__(self, torch, mgr, chunks):
        self.chunks = chunks
        self.data = b"".join(c.tobytes() for c in chunks)
        self.frames = [f.cpu().numpy().tobytes() for f in mgr.compress_batch([_dev(torch, c.tobytes()) for c in chunks])]
        self.cs = [len(f) for f in self.frames]
        self.ds = [len(c) for c in chunks]
        self.body = b"".join(self.frames)
        self.plain = self.body + table(self.cs, self.ds)
        self._ck = None

    @property
    def cks(self):
        if self._ck is None:
            self._ck = [xxh32lo(c.tobytes()) for c in self.chunks]
        return self._ck

    @property
    def checked(self):
        return self.body + table(self.cs, self.ds, self.cks)


@pytest.fixture(scope="module")
def case1(torch_cuda, mgr):
    return Case(torch_cuda, mgr, _chunks1())


@pytest.fixture(scope="module")
def case3(torch_cuda, mgr):
    rng = np.random.default_rng(2305)
    sizes = rng.integers(64, 2049, 2305)
    big = T.gen(T.DG_MIX, 48, 31, 65536)
    chunks, pos = [], 0
    for s in sizes:
        chunks.append(big[pos:pos + int(s)].copy())
        pos += int(s)
    return Case(torch_cuda, mgr, chunks)


def _check_packed(buf, size, status, cap, want):
    assert status == 0 and size == len(want), (status, size, len(want))
    assert buf[:size] == want
    assert buf[size:] == bytes([SENT]) * (len(buf) - size), "bytes past the stream were written"


# ---- 1, 2: pack is byte-exact; libzstd decodes the stream whole --------------------------------
@pytest.mark.parametrize("checksums", [False, True])
def test_pack_byte_exact(torch_cuda, case1, checksums):
    c = case1
    assert min(c.cs) < 16 and max(c.cs) > 40000 and any(o % 16 for o in np.cumsum(c.cs)[:-1])  # short frame, raw frame, odd offsets
    buf, size, status, cap = _pack(torch_cuda, c.chunks, checksums)
    _check_packed(buf, size, status, cap, c.checked if checksums else c.plain)


def test_libzstd_decodes_packed_stream(torch_cuda, case1, libzstd):
    buf, size, status, _ = _pack(torch_cuda, case1.chunks, True)
    assert status == 0
    assert T.zstd_decompress(buf[:size], len(case1.data)) == case1.data


# ---- 3: the scan crosses tiles -----------------------------------------------------------------
def test_scan_crosses_tiles(torch_cuda, case3):
    import cuda_zstd

    c = case3
    assert len(c.chunks) == 2305
    buf, size, status, cap = _pack(torch_cuda, c.chunks, False)
    _check_packed(buf, size, status, cap, c.plain)
    r = cuda_zstd.SeekableReader(_dev(torch_cuda, c.plain))
    assert (r.num_frames, r.size, r.max_frame, r.has_checksums) == (2305, int(np.sum(c.ds)), int(np.max(c.ds)), False)
    h = cuda_zstd.SeekableReader(c.plain)  # a host buffer: parsed on the host
    assert (h.num_frames, h.size, h.max_frame, h.has_checksums) == (2305, int(np.sum(c.ds)), int(np.max(c.ds)), False)


# ---- 4: compress_async then pack on one non-default stream, nothing in between ----------------
def test_composition_on_a_side_stream(torch_cuda, case1):
    s = torch_cuda.cuda.Stream()
    buf, size, status, cap = _pack(torch_cuda, case1.chunks, True, stream=s, sync_between=False)
    _check_packed(buf, size, status, cap, case1.checked)


def test_seekable_compress_and_reader(torch_cuda, case1, libzstd):
    import cuda_zstd

    data = np.frombuffer(case1.data, np.uint8)[: 3 * 65536 + 777]
    st = cuda_zstd.seekable_compress(_dev(torch_cuda, data.tobytes()), frame_size=65536, checksums=True)
    sb = st.cpu().numpy().tobytes()
    assert T.zstd_decompress(sb, len(data)) == data.tobytes()
    r = cuda_zstd.SeekableReader(st)
    assert (r.num_frames, r.size, r.has_checksums) == (4, len(data), True)
    assert r.read_all(verify=True).cpu().numpy().tobytes() == data.tobytes()
    assert r.read(65530, 70000).cpu().numpy().tobytes() == data[65530:135530].tobytes()
    assert cuda_zstd.SeekableReader(sb).read(5, 11) == data[5:16].tobytes()  # host bytes in, bytes out
    assert cuda_zstd.seekable_compress(data.tobytes(), checksums=True) == sb


# ---- 5: range reads ----------------------------------------------------------------------------
def _read(torch, dec, dstream, off, length, verify=False, temp_bytes=None, info=None):
    """cuda_zstd_seekable_read into the middle of a sentinel-filled buffer; returns (code,
    written, the length bytes) after checking that nothing around them was written."""
    import cuda_zstd

    L = cuda_zstd.lib()
    nf, mx = info
    need = L.cuda_zstd_seekable_read_get_temp_size(nf, mx) if temp_bytes is None else temp_bytes
    temp = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    out = torch.full((length + 2 * PAD,), SENT, dtype=torch.uint8, device="cuda")
    written = ctypes.c_size_t(12345)
    rc = L.cuda_zstd_seekable_read(dec._h, dstream.data_ptr(), dstream.numel(), off, length, out.data_ptr() + PAD, ctypes.byref(written),
                                   1 if verify else 0, temp.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o = out.cpu().numpy().tobytes()
    assert o[:PAD] == bytes([SENT]) * PAD and o[PAD + length:] == bytes([SENT]) * PAD, "the read wrote outside d_out"
    return rc, written.value, o[PAD:PAD + length]


def _ranges(ds):
    """The issue's range set for frames of content sizes ds (zero-size entries allowed)."""
    total = int(np.sum(ds))
    bounds = [int(b) for b in np.cumsum(ds)[:-1] if 0 < b < total]
    nz = [(int(s), int(d)) for s, d in zip(np.cumsum([0] + list(ds[:-1])), ds) if d > 0]
    big = max(nz, key=lambda p: p[1])
    out = [(0, total), (0, 1), (total - 1, 1), (big[0] + big[1] // 3, max(1, big[1] // 3)), big]
    picks = sorted(set(bounds[:: max(1, len(bounds) // 5)] + bounds[-1:]))
    out += [(b - 1, 2) for b in picks]
    a = nz[1][0] + 1 if nz[1][1] > 2 else nz[1][0]  # odd offset inside the second frame with content
    k = min(len(nz) - 1, 5)
    out.append((a | 1, nz[k][0] + max(1, nz[k][1] // 2) - (a | 1)))  # ends inside a later frame: >= 3 frames, both edges partial
    out.append((total // 2, 0))
    return out


def _check_ranges(torch, dec, stream_bytes, data, ds, verify):
    d = _dev(torch, stream_bytes)
    info = (len(ds), int(np.max(ds)))
    for off, length in _ranges(ds):
        rc, w, got = _read(torch, dec, d, off, length, verify, info=info)
        assert (rc, w) == (0, length), (off, length, rc)
        assert got == data[off:off + length], (off, length)
    total = len(data)
    rc, w, got = _read(torch, dec, d, total - 9, 10, verify, info=info)  # offset + length == total + 1
    assert (rc, w) == (INVALID, 0) and got == bytes([SENT]) * 10


@pytest.mark.parametrize("verify", [False, True])
def test_range_reads_case1(torch_cuda, dec, case1, verify):
    c = case1
    r = _ranges(c.ds)
    assert any(sum(1 for s, e in zip(np.cumsum([0] + c.ds[:-1]), np.cumsum(c.ds)) if s < o + n and e > o) >= 3 for o, n in r if n)
    _check_ranges(torch_cuda, dec, c.checked, c.data, c.ds, verify)
    if not verify:
        _check_ranges(torch_cuda, dec, c.plain, c.data, c.ds, True)  # verify on a table without checksums: nothing to check


def test_range_reads_case3(torch_cuda, dec, case3):
    _check_ranges(torch_cuda, dec, case3.plain, case3.data, case3.ds, False)


def test_read_temp_too_small(torch_cuda, dec, case1):
    import cuda_zstd

    c = case1
    d = _dev(torch_cuda, c.plain)
    info = (len(c.ds), max(c.ds))
    need = cuda_zstd.lib().cuda_zstd_seekable_read_get_temp_size(*info)
    for tb in (16, need // 2):
        rc, w, got = _read(torch_cuda, dec, d, 0, len(c.data), temp_bytes=tb, info=info)
        assert (rc, w) == (TOO_SMALL, 0) and got == bytes([SENT]) * len(c.data)


# ---- 6: a foreign stream -----------------------------------------------------------------------
def test_foreign_stream(torch_cuda, dec, libzstd):
    datas = [T.gen(T.DG_TEXT, 1, 61, 50000), T.gen(T.DG_JSON, 1, 62, 70001), T.gen(T.DG_MIX, 1, 63, 33333), np.zeros(0, np.uint8),
             T.gen(T.DG_SOURCE, 1, 64, 20000), None, T.gen(T.DG_EXE, 1, 65, 4097)]
    opts = [dict(level=1), dict(level=3, checksum=True), dict(level=19, content_size=False), dict(level=3), dict(level=19), None, dict(level=1)]
    skip = struct.pack("<II", 0x184D2A53, 7) + b"metadat"
    frames = [skip if o is None else T.zstd_compress(d, **o) for d, o in zip(datas, opts)]
    contents = [b"" if d is None else d.tobytes() for d in datas]
    ds = [len(c) for c in contents]
    data = b"".join(contents)
    cs = [len(f) for f in frames]
    for cks in (None, [xxh32lo(c) for c in contents]):
        s = b"".join(frames) + table(cs, ds, cks)
        assert T.zstd_decompress(s, len(data)) == data
        _check_ranges(torch_cuda, dec, s, data, ds, cks is not None)


# ---- 7: damaged tables -------------------------------------------------------------------------
def test_damaged_tables(torch_cuda, dec, case1):
    c = case1
    n, total, good = len(c.ds), len(c.data), c.checked
    tab = len(good) - (n * 12 + 17)  # the table's first byte
    info = (n, max(c.ds))

    def patched(pos, fmt, v):
        b = bytearray(good)
        struct.pack_into(fmt, b, pos, v)
        return bytes(b)

    k = 1  # a 65536-byte frame
    cases = {
        "seekable magic": (patched(len(good) - 4, "<I", 0x8F92EAB0), CORRUPT),
        "reserved bit": (patched(len(good) - 5, "<B", 0x80 | 0x10), CORRUPT),
        "frame size": (patched(tab + 4, "<I", n * 12 + 9 + 12), CORRUPT),
        "csize sum": (patched(tab + 8, "<I", c.cs[0] + 1), CORRUPT),
        "n too large": (patched(len(good) - 9, "<I", 0x7FFFFFF), CORRUPT),
        "dsize short": (patched(tab + 8 + 12 * k + 4, "<I", c.ds[k] - 1), TOO_SMALL),
    }
    for name, (s, want) in cases.items():
        length = total - 1 if name == "dsize short" else total
        rc, w, got = _read(torch_cuda, dec, _dev(torch_cuda, s), 0, length, True, info=info)
        assert (rc, w) == (want, 0), name
        if want == CORRUPT:
            assert got == bytes([SENT]) * length, name
    flipped = patched(tab + 8 + 12 * k + 8, "<I", c.cks[k] ^ 1)
    d = _dev(torch_cuda, flipped)
    rc, w, got = _read(torch_cuda, dec, d, 0, total, True, info=info)
    assert (rc, w) == (CHECKSUM, 0)
    rc, w, got = _read(torch_cuda, dec, d, 0, total, False, info=info)
    assert (rc, w) == (0, total) and got == c.data
    rc, w, got = _read(torch_cuda, dec, d, 65536 + 100, 50, True, info=info)  # the edge frame is verified whole
    assert (rc, w) == (CHECKSUM, 0)


# ---- 8: pack errors ----------------------------------------------------------------------------
def test_pack_errors(torch_cuda, case1, libzstd):
    c = case1
    buf, size, status, cap = _pack(torch_cuda, c.chunks, False, cap_delta=(len(c.plain), -1))
    assert (size, status) == (0, TOO_SMALL) and buf == bytes([SENT]) * len(buf)
    buf, size, status, cap = _pack(torch_cuda, c.chunks, False, cap_delta=(len(c.plain), 0))
    _check_packed(buf, size, status, cap, c.plain)
    buf, size, status, cap = _pack(torch_cuda, c.chunks, False, bad_status=(3, CORRUPT))
    assert (size, status) == (0, CORRUPT) and buf == bytes([SENT]) * len(buf)
    buf, size, status, cap = _pack(torch_cuda, [], False)
    assert status == 0 and size == 17 and buf[:17] == table([], [])
    assert buf[17:] == bytes([SENT]) * (len(buf) - 17)
    assert T.zstd_decompress(buf[:17], 0) == b""

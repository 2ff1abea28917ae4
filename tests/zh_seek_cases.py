"""Builders shared by the tests of the batched range read of a seekable stream: seek tables
written with `struct` (a restatement of the format that shares no code with the library), the
seeded chunks of the three test streams, and one runner for cuda_zstd_seekable_read_ranges that
surrounds every destination with sentinel bytes.

    u32 0x184D2A5E | u32 N*E + 9 | N x { u32 csize; u32 dsize; [u32 xxh64 low 32] } | u32 N |
    u8 descriptor (bit 7: checksums) | u32 0x8F92EAB1          (little-endian; E = 8 or 12)"""
import ctypes
import struct

import numpy as np

import zh_testlib as T

INVALID, CORRUPT, TOO_SMALL, CHECKSUM = 2, 6, 7, 10
SENT = 0xA5
PAD = 64
STATUS_SENT = -77

EMPTY_FRAME = bytes([0x28, 0xB5, 0x2F, 0xFD, 0x20, 0x00, 0x01, 0x00, 0x00])  # single segment, content size 0, one last raw block of 0 bytes


def skippable(payload=b"meta"):
    return struct.pack("<II", 0x184D2A53, len(payload)) + payload


def table(csizes, dsizes, cks=None):
    n, e = len(csizes), 8 if cks is None else 12
    out = struct.pack("<II", 0x184D2A5E, n * e + 9)
    for k in range(n):
        out += struct.pack("<II", csizes[k], dsizes[k])
        if cks is not None:
            out += struct.pack("<I", cks[k])
    return out + struct.pack("<IBI", n, 0x80 if cks is not None else 0, 0x8F92EAB1)


def xxh32lo(b):
    a = np.frombuffer(bytes(b), np.uint8).copy() if len(b) else np.zeros(1, np.uint8)
    return int(T.oracle().orc_xxh64(a.ctypes.data, len(b))) & 0xFFFFFFFF


def dev(torch, b):
    a = np.frombuffer(bytes(b), np.uint8).copy()
    return torch.from_numpy(a if a.size else np.zeros(1, np.uint8)).cuda()[: len(b)]


# ---- the seeded content of the streams ---------------------------------------------------------
def data_a():
    """150,000 bytes: text, then mixed content."""
    return np.concatenate([T.gen(T.DG_TEXT, 1, 0xA11CE, 65536), T.gen(T.DG_MIX, 1, 0xA11CF, 65536), T.gen(T.DG_TEXT, 1, 0xA11D0, 18928)])


def data_b():
    """1,100 x 256 bytes."""
    return T.gen(T.DG_MIX, 1, 0xB0B, 1100 * 256)


def chunks_c():
    """Three pieces of content for the hand-assembled stream."""
    return [T.gen(T.DG_TEXT, 1, 0xC0, 3000), T.gen(T.DG_MIX, 1, 0xC1, 4097), T.gen(T.DG_JSON, 1, 0xC2, 511)]


def split(data, frame_size):
    return [data[o:o + frame_size] for o in range(0, len(data), frame_size)]


class Stream:
    """A seekable stream put together on the host from given frames: frames[k] holds
    contents[k] (b"" for an entry of size 0)."""

    def __init__(self, frames, contents, checksums):
        self.frames = [bytes(f) for f in frames]
        self.contents = [bytes(c) for c in contents]
        self.cs = [len(f) for f in self.frames]
        self.ds = [len(c) for c in self.contents]
        self.data = b"".join(self.contents)
        self.cks = [xxh32lo(c) for c in self.contents] if checksums else None
        self.bytes = b"".join(self.frames) + table(self.cs, self.ds, self.cks)
        self.entry = 12 if checksums else 8
        self.table_at = len(self.bytes) - (len(self.frames) * self.entry + 17)
        self.starts = [int(v) for v in np.cumsum([0] + self.ds[:-1])]
        self.cstarts = [int(v) for v in np.cumsum([0] + self.cs[:-1])]
        self.total = len(self.data)
        self.info = (len(self.ds), max(self.ds) if self.ds else 0)

    def patched(self, pos, fmt, v):
        b = bytearray(self.bytes)
        struct.pack_into(fmt, b, pos, v)
        return bytes(b)

    def touched(self, ranges, max_length=None):
        """Indices of the frames with content under the valid, non-empty ranges."""
        out = set()
        for off, n in ranges:
            if n == 0 or off + n > self.total or (max_length is not None and n > max_length):
                continue
            out |= {k for k, (s, d) in enumerate(zip(self.starts, self.ds)) if d and s < off + n and s + d > off}
        return out


def compress_frames(torch, mgr, chunks):
    """Level-3 frames of the chunks from the GPU compressor (mgr: cuda_zstd.Manager(3))."""
    return [f.cpu().numpy().tobytes() for f in mgr.compress_batch([dev(torch, np.asarray(c).tobytes()) for c in chunks])]


# ---- the runner ------------------------------------------------------------------------------------
class Result:
    pass


def read_ranges(torch, dec, stream_bytes, info, ranges, verify=0, max_length=None, max_jobs=None, temp_delta=0, dst_offsets=None, arena_bytes=None,
                dstream=None):
    """cuda_zstd_seekable_read_ranges over `ranges` [(offset, length)]: every destination lies in
    one sentinel-filled arena, PAD bytes apart (or at dst_offsets), and the statuses start as
    STATUS_SENT.  Returns rc, statuses, frames_decoded, the bytes of each destination, and
    `clean`: whether every byte of the arena outside the destinations still holds the sentinel.
    info: (num_frames, max_frame_uncompressed); max_jobs: what the temp is sized for (default:
    every frame); temp_delta: added to the temp size handed to the call."""
    import cuda_zstd

    L = cuda_zstd.lib()
    r = len(ranges)
    lens = [n for _, n in ranges]
    if dst_offsets is None:
        dst_offsets, pos = [], PAD
        for n in lens:
            dst_offsets.append(pos)
            pos += min(n, 1 << 20) + PAD  # (an invalid range may name an absurd length)
        arena_bytes = pos
    d = dev(torch, stream_bytes) if dstream is None else dstream
    arena = torch.full((arena_bytes,), SENT, dtype=torch.uint8, device="cuda")
    d_off = torch.tensor([o for o, _ in ranges], dtype=torch.int64).cuda() if r else torch.zeros(1, dtype=torch.int64, device="cuda")
    d_len = torch.tensor(lens, dtype=torch.int64).cuda() if r else torch.zeros(1, dtype=torch.int64, device="cuda")
    d_ptr = torch.tensor([arena.data_ptr() + o for o in dst_offsets], dtype=torch.int64).cuda() if r else torch.zeros(1, dtype=torch.int64, device="cuda")
    d_st = torch.full((max(r, 1),), STATUS_SENT, dtype=torch.int32, device="cuda")
    ml = max(lens, default=0) if max_length is None else max_length
    need = L.cuda_zstd_seekable_read_ranges_get_temp_size(info[0], r, info[0] if max_jobs is None else max_jobs, info[1]) + temp_delta
    temp = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    fd = ctypes.c_size_t(12345)
    torch.cuda.synchronize()
    res = Result()
    res.rc = L.cuda_zstd_seekable_read_ranges(dec._h, d.data_ptr(), len(stream_bytes), d_off.data_ptr(), d_len.data_ptr(), d_ptr.data_ptr(), r, ml,
                                              verify, d_st.data_ptr(), ctypes.byref(fd), temp.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    a = arena.cpu().numpy()
    res.statuses = [int(v) for v in d_st.cpu()[:r]]
    res.frames_decoded = fd.value
    keep = np.ones(arena_bytes, bool)
    res.got = []
    for o, n in zip(dst_offsets, lens):
        n = min(n, arena_bytes - o)
        res.got.append(a[o:o + n].tobytes())
        keep[o:o + n] = False
    res.clean = bool((a[keep] == SENT).all())
    res.arena = a
    return res


def check(res, stream, ranges, failed=(), max_length=None):
    """rc 0, nothing outside the destinations written, the ranges in `failed` {index: code}
    carry that code and an all-sentinel destination, every other range is exact."""
    assert res.rc == 0, res.rc
    assert res.clean, "bytes outside the destinations were written"
    failed = dict(failed)
    for k, (off, n) in enumerate(ranges):
        if k in failed:
            assert res.statuses[k] == failed[k], (k, off, n, res.statuses[k])
            assert res.got[k] == bytes([SENT]) * len(res.got[k]), ("a failed range's destination was written", k)
        else:
            assert res.statuses[k] == 0, (k, off, n, res.statuses[k])
            assert res.got[k] == stream.data[off:off + n], (k, off, n)

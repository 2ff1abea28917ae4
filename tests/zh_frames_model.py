"""Plain-Python model of the frame index (cuda_zstd_seekable_index; test infrastructure: no GPU).

walk(buf) is the serial walk over a buffer of concatenated frames as csrc/zh_frames.h states it
(the decoder's frame_header checks and the extent-only block hop): the frames, and where and how
the walk stops.  index(buf, ...) is the whole call on top of it: return code, *num_frames,
*error_offset and the table's bytes.

Builders: libzstd frames come from zh_testlib.zstd_compress; skippable(), hand_frame() and
pad_until() are assembled here byte by byte, so a frame start can sit at any offset and a payload
can hold any bytes (magics included)."""
import struct
from collections import namedtuple

import numpy as np

import zh_size_model as M
import zh_testlib as T

MAGIC = 0xFD2FB528
SKIP_MAGIC = 0x184D2A50
BLOCK_MAX = 128 * 1024
MAX_FRAMES, MAX_FIELD = 0x8000000, 0x40000000
TILE, LANE = 4096, 16  # zh_frames.h: the scan kernels' tile and one lane's bytes
OK, BAD_MAGIC, CORRUPT = 0, 5, 6  # the walk's statuses (the decoder's)
CODE = {OK: 0, BAD_MAGIC: 1, CORRUPT: 6}  # the nvcomp-style codes the C ABI returns for them
INVALID, TOO_SMALL, DICT_WRONG = 2, 7, 1

Frame = namedtuple("Frame", "off size skippable fcs")  # fcs None: not stated
Walk = namedtuple("Walk", "frames status err_off")
Index = namedtuple("Index", "rc num_frames error_offset table")


def candidates(max_frames):
    """Candidates the temp buffer of a call with max_frames holds (ZH_FRAMES_CANDIDATES)."""
    return 2 * min(max_frames, MAX_FRAMES) + 1024


# ---- the walk ---------------------------------------------------------------------------------
def span(b, off, first):
    """The frame at b[off:] -> (status, Frame or None)."""
    n = len(b) - off
    if n < 4:
        return CORRUPT, None
    magic = int.from_bytes(b[off:off + 4], "little")
    if magic & 0xFFFFFFF0 == SKIP_MAGIC:
        if n < 8:
            return CORRUPT, None
        size = 8 + int.from_bytes(b[off + 4:off + 8], "little")
        return (CORRUPT, None) if size > n else (OK, Frame(off, size, True, 0))
    if magic != MAGIC:
        return (BAD_MAGIC if first else CORRUPT), None
    if n < 5:
        return CORRUPT, None
    fhd = b[off + 4]
    fcsf, single, chk, didf = fhd >> 6, (fhd >> 5) & 1, (fhd >> 2) & 1, fhd & 3
    if fhd & 8:
        return CORRUPT, None
    didn, fcsn = (0, 1, 2, 4)[didf], (single, 2, 4, 8)[fcsf]
    ip = 5 + (0 if single else 1) + didn + fcsn
    if n < ip:
        return CORRUPT, None
    q = off + 5
    if not single:
        if 10 + (b[q] >> 3) > 30:
            return CORRUPT, None
        q += 1
    q += didn
    fcs = int.from_bytes(b[q:q + fcsn], "little") + (256 if fcsn == 2 else 0) if fcsn else None
    if fcs == (1 << 64) - 1:  # the decoder's "absent" value
        fcs = None
    while True:
        if n - ip < 3:
            return CORRUPT, None
        bh = int.from_bytes(b[off + ip:off + ip + 3], "little")
        last, bt, bsz = bh & 1, (bh >> 1) & 3, bh >> 3
        ip += 3
        body = 1 if bt == 1 else bsz
        if bt == 3 or (bt == 2 and bsz >= BLOCK_MAX) or n - ip < body:
            return CORRUPT, None
        ip += body
        if last:
            break
    if chk:
        if n - ip < 4:
            return CORRUPT, None
        ip += 4
    return OK, Frame(off, ip, False, fcs)


def walk(buf):
    b = bytes(buf)
    frames, ip = [], 0
    while ip < len(b):
        st, f = span(b, ip, ip == 0)
        if st != OK:
            return Walk(frames, st, ip)
        frames.append(f)
        ip += f.size
    return Walk(frames, OK, 0)


def frame_dict_id(fr):
    fhd = fr[4]
    didn = (0, 1, 2, 4)[fhd & 3]
    q = 5 + (0 if (fhd >> 5) & 1 else 1)
    return int.from_bytes(fr[q:q + didn], "little")


def sized(fr, dictionary=None):
    """A size job: (size, code) of one frame without a Frame_Content_Size, by the size pass's model."""
    did = frame_dict_id(fr)
    if did and (not dictionary or M.dict_layout(dictionary)[0] != did):
        return 0, DICT_WRONG
    n, ok = M.size(fr, dictionary)
    return (n, 0) if ok else (0, CORRUPT)


def table(entries):
    """The seek table of [(Compressed_Size, Decompressed_Size)], descriptor 0."""
    body = b"".join(struct.pack("<II", c, d) for c, d in entries)
    return struct.pack("<II", 0x184D2A5E, len(body) + 9) + body + struct.pack("<IB", len(entries), 0) + struct.pack("<I", 0x8F92EAB1)


def index(buf, max_frames=None, table_capacity=None, dictionary=None):
    """The call's results for a non-empty stream and a sufficient temp buffer."""
    b = bytes(buf)
    w = walk(b)
    nf = len(w.frames)
    if w.status != OK:
        return Index(CODE[w.status], nf, w.err_off, b"")
    if max_frames is not None and nf > min(max_frames, MAX_FRAMES):
        return Index(TOO_SMALL if nf <= MAX_FRAMES else INVALID, nf, 0, b"")
    if any(f.size > MAX_FIELD or (f.fcs or 0) > MAX_FIELD for f in w.frames):
        return Index(INVALID, nf, 0, b"")
    if table_capacity is not None and table_capacity < 17 + 8 * nf:
        return Index(TOO_SMALL, nf, 0, b"")
    entries = []
    for i, f in enumerate(w.frames):
        d = f.fcs
        if d is None:
            d, code = sized(b[f.off:f.off + f.size], dictionary)
            if code:
                return Index(code, i, f.off, b"")
        entries.append((f.size, d))
    if any(d > MAX_FIELD for _, d in entries):
        return Index(INVALID, nf, 0, b"")
    return Index(0, nf, 0, table(entries))


# ---- builders ---------------------------------------------------------------------------------
def skippable(payload=b"", nibble=0):
    return struct.pack("<II", SKIP_MAGIC | nibble, len(payload)) + bytes(payload)


def pad_until(prefix, offset, nibble=0, fill=0x55):
    """prefix + one skippable frame that ends exactly at `offset`: whatever comes next starts there."""
    gap = offset - len(prefix)
    assert gap >= 8, "a skippable frame takes at least 8 bytes"
    return bytes(prefix) + skippable(bytes([fill]) * (gap - 8), nibble)


def raw_block(payload, last=False):
    assert len(payload) <= BLOCK_MAX
    return (int(last) | 0 << 1 | len(payload) << 3).to_bytes(3, "little") + bytes(payload)


def rle_block(byte, n, last=False):
    assert n <= BLOCK_MAX
    return (int(last) | 1 << 1 | n << 3).to_bytes(3, "little") + bytes([byte])


def header(fcs=None, fcs_bytes=None, single=False, checksum=False, dict_id=0, window_byte=0x38, reserved=False):
    """Frame header bytes (magic included).  fcs_bytes 1/2/4/8 picks the field (default: the smallest)."""
    fcsn = 0
    if fcs is not None:
        fcsn = fcs_bytes or (1 if fcs < 256 and single else 2 if 256 <= fcs < 65792 else 4 if fcs < 1 << 32 else 8)
    assert fcsn != 1 or single
    didn = 0 if not dict_id else 1 if dict_id < 256 else 2 if dict_id < 65536 else 4
    fhd = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcsn] << 6 | int(single) << 5 | int(reserved) << 3 | int(checksum) << 2 | {0: 0, 1: 1, 2: 2, 4: 3}[didn]
    out = struct.pack("<IB", MAGIC, fhd) + (b"" if single else bytes([window_byte])) + dict_id.to_bytes(didn, "little")
    if fcsn:
        out += (fcs - (256 if fcsn == 2 else 0)).to_bytes(fcsn, "little")
    return out


def hand_frame(payload, stated=True, block=BLOCK_MAX, **hdr):
    """A frame of raw blocks holding `payload` verbatim (no checksum): decodes to the payload."""
    payload = bytes(payload)
    cuts = list(range(0, len(payload), block)) or [0]
    blocks = b"".join(raw_block(payload[c:c + block], c == cuts[-1]) for c in cuts)
    return header(fcs=len(payload) if stated else None, **hdr) + blocks


def rle_frame(byte, n, stated=True, **hdr):
    reps = [BLOCK_MAX] * (n // BLOCK_MAX) + ([n % BLOCK_MAX] if n % BLOCK_MAX or n == 0 else [])
    blocks = b"".join(rle_block(byte, r, i == len(reps) - 1) for i, r in enumerate(reps))
    return header(fcs=n if stated else None, **hdr) + blocks


EMPTY = hand_frame(b"", single=True)  # 9 bytes: the smallest Zstandard frame


# ---- content and the shared vectors --------------------------------------------------------------
def text(n, seed=1):
    """n compressible bytes."""
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, int(k), dtype=np.uint8)) for k in rng.integers(2, 9, 64)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, 64))] + b" "
    return bytes(out[:n])


def noise(n, seed=2):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def magics():
    """The 17 four-byte strings the scan takes for a frame start."""
    return [struct.pack("<I", MAGIC)] + [struct.pack("<I", SKIP_MAGIC | k) for k in range(16)]


_cache = {}


def _once(name, make):
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def variety():
    """[(bytes, content)] frames of every header and block kind; content None: not decodable
    without more (none here)."""
    def make():
        out = []
        for n in (0, 255, 256, 65791, 65792, 70000):  # every Frame_Content_Size width libzstd writes
            d = text(n, n + 3)
            out.append((T.zstd_compress(d), d))
        d = b"\x07" * 5
        out.append((hand_frame(d, single=True, fcs_bytes=8), d))  # the 8-byte field
        d = text(3000, 11)
        out.append((T.zstd_compress(d, content_size=False), d))
        out.append((T.zstd_compress(d, checksum=True), d))
        out.append((T.zstd_compress(d, checksum=True, content_size=False), d))
        out.append((T.zstd_compress(d, window_log=20), d))  # not single-segment: a window descriptor
        out.append((T.zstd_compress(b""), b""))
        out.append((T.zstd_compress(b"", content_size=False), b""))
        d = text(300 * 1024, 12)
        out.append((T.zstd_compress(d), d))  # three blocks
        out.append((T.zstd_compress(d, content_size=False, checksum=True), d))
        d = bytes(200000)
        out.append((T.zstd_compress(d), d))
        out.append((rle_frame(0, 200000), d))  # RLE blocks
        out.append((rle_frame(9, 1000, stated=False), b"\x09" * 1000))
        d = noise(5000)
        out.append((T.zstd_compress(d), d))  # a raw block
        out.append((hand_frame(d, stated=False, block=1777), d))
        return out
    return _once("variety", make)


def variety_stream():
    """-> (stream, content): the variety frames with skippable frames of length 0 and 1 and all 16
    magics in front of, between and behind them."""
    def make():
        fr = variety()
        parts, content = [skippable(b"", 0), skippable(b"x", 1)], b""
        for i, (f, d) in enumerate(fr):
            parts.append(f)
            content += d
            if i < 16:
                parts.append(skippable(b"" if i % 2 else b"y", i))
        parts += [skippable(b"", 15), skippable(b"z", 14)]
        return b"".join(parts), content
    return _once("variety_stream", make)


def tile_edge_streams():
    """[(name, stream, content)]: a frame start at each of T-4 .. T+1 for T the first and second
    tile boundary, and at 16-byte lane boundaries +-3."""
    def make():
        d = text(100, 21)
        f = T.zstd_compress(d)
        out = []
        spots = [t + k for t in (TILE, 2 * TILE) for k in range(-4, 2)] + [b + k for b in (LANE * 7, TILE + LANE * 3) for k in range(-3, 4)]
        for s in spots:
            st = pad_until(EMPTY, s, nibble=s % 16) + f + EMPTY
            out.append((f"start_{s}", st, d))
        # both boundaries in one stream, the second start right behind a frame that straddles the first
        st = pad_until(b"", TILE - 3) + f
        st = pad_until(st, 2 * TILE - 1, nibble=3) + f + skippable(b"q")
        out.append(("two_tiles", st, d + d))
        return out
    return _once("tile_edges", make)


def false_candidate_streams():
    """[(name, stream, content)]: magics where no frame of the stream starts."""
    def make():
        d = text(500, 31)
        f = T.zstd_compress(d)
        ms = b"".join(m + b"\x00" for m in magics())
        nested = T.zstd_compress(text(200, 32))
        # a nested frame header whose blocks run past the stream's end: a raw block of 2^20 bytes
        runaway = header(fcs=None) + (0 | 0 << 1 | (1 << 20) << 3).to_bytes(3, "little")
        out = [
            ("magics_in_skippable", f + skippable(ms * 3) + f, d + d),
            ("magics_in_raw_block", f + hand_frame(ms * 40, single=True) + f, d + ms * 40 + d),
            ("frame_in_skippable", skippable(nested + nested, 7) + f + skippable(b"ab" + nested), d),
            # ... and a nested skippable header that claims two bytes more than the stream has left
            ("runaway_in_skippable", f + skippable(runaway + b"\x00" * 20) + f + skippable(struct.pack("<II", SKIP_MAGIC | 5, 6) + b"1234"), d + d),
            ("runaway_skippable_in_raw", hand_frame(struct.pack("<II", SKIP_MAGIC, 0xFFFFFFF0) + b"tail", single=True) + f,
             struct.pack("<II", SKIP_MAGIC, 0xFFFFFFF0) + b"tail" + d),
        ]
        return out
    return _once("false_candidates", make)


def end_magic_streams():
    """[(name, stream, content)]: the stream's last bytes spell the start of a magic (a stated
    payload, so the stream is well formed): positions whose four bytes would pass the end."""
    d = text(300, 33)
    f = T.zstd_compress(d)
    m = struct.pack("<I", MAGIC)
    return [(f"magic_tail_{k}", f + skippable(b"pad" + m[:k]), d) for k in (1, 2, 3)] + [("magic_last4", f + skippable(m), d)]


def count_streams():
    """[(n, stream, content)] for the doubling rounds: n frames, empty and tiny alternating."""
    def make():
        small = [text(40 + 23 * i, 70 + i) for i in range(7)]  # frames of 50 to 150 bytes: 5,000 make ~300 KiB
        tiny = [T.zstd_compress(d) for d in small]
        out = []
        for n in (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 5000):
            parts, content = [], []
            for i in range(n):
                if i % 3 == 1:
                    parts.append(EMPTY)
                else:
                    parts.append(tiny[i % 7])
                    content.append(small[i % 7])
            out.append((n, b"".join(parts), b"".join(content)))
        return out
    return _once("counts", make)


def malformed_streams():
    """[(name, stream)]: each fails in the walk (never in a size job)."""
    def make():
        d = text(2000, 41)
        good = T.zstd_compress(d) + skippable(b"mid", 2)
        ck = T.zstd_compress(d, checksum=True)  # magic 4 | header 2.. | block header 3 | body | checksum 4
        hdr = 5 + (0 if ck[4] >> 5 & 1 else 1) + (ck[4] >> 5 & 1, 2, 4, 8)[ck[4] >> 6]  # its header's length (no Dictionary_ID)
        out = [("cut_in_magic", good + ck[:2]), ("cut_in_header", good + ck[:5]), ("cut_in_block_header", good + ck[:hdr + 2]),
               ("cut_in_block_body", good + ck[:hdr + 3 + 10]), ("cut_in_checksum", good + ck[:-2]), ("cut_whole_checksum", good + ck[:-4])]
        for k in (1, 2, 3, 8):
            out.append((f"garbage_{k}", good + ck + b"\xa5" * k))
        out.append(("block_type_3", good + header(fcs=4, single=True) + (1 | 3 << 1 | 4 << 3).to_bytes(3, "little") + b"abcd" + good))
        out.append(("reserved_bit", good + header(fcs=4, single=True, reserved=True) + raw_block(b"abcd", True)))
        # (Window_Log 32: over libzstd's limit of 31 too; the decoder's own, 30, is pinned apart)
        out.append(("window_over_limit", good + header(fcs=4, window_byte=22 << 3) + raw_block(b"abcd", True) + good))
        out.append(("compressed_block_128k", good + header(fcs=4, single=True) + (1 | 2 << 1 | BLOCK_MAX << 3).to_bytes(3, "little") + bytes(BLOCK_MAX)))
        out.append(("wrong_first_magic", b"\x00\x01\x02\x03" + good))
        out.append(("wrong_first_magic_short", b"\x28\xb5"))
        out.append(("skippable_past_end", good + skippable(b"abcdef")[:-1]))
        out.append(("skippable_header_cut", good + skippable(b"")[:6]))
        out.append(("no_last_block", good + header(fcs=4, single=True) + raw_block(b"abcd", False)))
        return out
    return _once("malformed", make)


def good_streams():
    """[(name, stream, content)]: every well-formed vector."""
    vs, vc = variety_stream()
    return ([("variety", vs, vc)] + tile_edge_streams() + false_candidate_streams() + end_magic_streams()
            + [(f"count_{n}", s, c) for n, s, c in count_streams()])

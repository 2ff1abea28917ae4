"""Long-distance matching, restated in numpy (the rules of csrc/zh_ldm.h and csrc/zh_ldm.hip).

hash -> samples (per-cell cap) -> earliest-wins table -> candidates -> first distinct distances ->
longest run per distance -> the cell's split -> the frame's partition, plus the bytes of a
one-sequence block built from the RFC 8878 predefined tables.  The GPU tests compare
cuda_zstd.ldm_plan against `plan`, the CPU tests decode `model_frame` with libzstd."""
import numpy as np

HASH_BYTES = 64
RATE_LOG = 7
CELL = 32768
CELL_SAMPLES = 512
CELL_OFFSETS = 4
MIN_SEG = 1024
MIN_DIST = 32768  # exclusive
MAX_DIST = (1 << 29) - 4
BLOCK_MAX = 16
SEG = 128  # the run search is exact for runs of at least SEG bytes (shorter ones never matter: MIN_SEG >= 2 SEG)

U64 = np.uint64
M64 = (1 << 64) - 1


def g(byte):
    x = ((byte + 1) * 0x9E3779) & 0xFFFFFFFF
    y = (x ^ (x >> 13)) & 0xFFFFFF
    hi = (y * 0x85EBCA) & 0xFFFFFFFF
    lo = ((y ^ 0xC2B2AE) * 0x27D4EB) & 0xFFFFFFFF
    return hi << 32 | lo


G = np.array([g(b) for b in range(256)], dtype=U64)


def hash_at(buf, p):
    """Scalar hash of the 64 bytes at p (python ints)."""
    h = 0
    for i in range(HASH_BYTES):
        h = ((h << 1) + g(int(buf[p + i]))) & M64
    return h


def hashes(data):
    """h of every position p with p + 64 <= len(data) (uint64 array; empty when shorter)."""
    data = np.asarray(data, dtype=np.uint8)
    m = len(data) - HASH_BYTES + 1
    if m <= 0:
        return np.zeros(0, dtype=U64)
    h = np.zeros(m, dtype=U64)
    for i in range(HASH_BYTES):
        h = (h << U64(1)) + G[data[i:i + m]]
    return h


def is_sample(h):
    h = np.asarray(h, dtype=U64)
    m = ((h >> U64(32)) * U64(0x9E3779B1) + (h & U64(0xFFFFFFFF)) * U64(0x85EBCA77)) & U64(0xFFFFFFFF)
    return (m >> U64(32 - RATE_LOG)) == U64((1 << RATE_LOG) - 1)


def slot_of(h, table_log):
    return ((np.asarray(h, dtype=U64) * U64(0x9E3779B185EBCA87)) >> U64(64 - table_log)).astype(np.int64)


def tag_of(h):
    h = np.asarray(h, dtype=U64)
    return ((h ^ (h >> U64(32))) * U64(0xC2B2AE3D27D4EB4F)) >> U64(32)


def table_log(frame_bytes, hash_log):
    cl = 0
    while cl < 63 and (1 << cl) < frame_bytes:
        cl += 1
    want = max(10, cl + 1 - RATE_LOG)
    return min(want, min(max(hash_log, 10), 30))


def max_dist(window_log):
    return MAX_DIST if window_log >= 29 else 1 << window_log


def kept_samples(data):
    """Positions of the kept samples (ascending) and their hashes: per cell, the first CELL_SAMPLES."""
    h = hashes(data)
    pos = np.flatnonzero(is_sample(h))
    if len(pos) == 0:
        return pos, h[pos]
    cell = pos // CELL
    first = np.searchsorted(cell, cell, side="left")  # index of each cell's first sample
    keep = (np.arange(len(pos)) - first) < CELL_SAMPLES
    pos = pos[keep]
    return pos, h[pos]


def build_table(pos, h, tlog):
    """Earliest position per slot: min of (pos << 32 | tag)."""
    table = np.full(1 << tlog, M64, dtype=U64)
    if len(pos):
        keys = (pos.astype(U64) << U64(32)) | tag_of(h)
        np.minimum.at(table, slot_of(h, tlog), keys)
    return table


def longest_run(eq):
    """(start, length) of the longest run of True in eq, lowest start on ties; (0, 0) if none."""
    if not eq.any():
        return 0, 0
    x = np.concatenate(([0], eq.astype(np.int8), [0]))
    d = np.diff(x)
    starts = np.flatnonzero(d == 1)
    ends = np.flatnonzero(d == -1)
    lens = ends - starts
    k = int(np.argmax(lens))  # first maximum = lowest start
    return int(starts[k]), int(lens[k])


def plan(data, window_log=27, hash_log=20, min_seg=MIN_SEG):
    """Records (seg_start, seg_len, distance) per cell, uint32 [cells, 3]; seg_len 0 = unsplit."""
    data = np.asarray(data, dtype=np.uint8)
    n = len(data)
    ncell = (n + CELL - 1) // CELL
    rec = np.zeros((ncell, 3), dtype=np.uint32)
    pos, h = kept_samples(data)
    tlog = table_log(n, hash_log)
    table = build_table(pos, h, tlog)
    slots = slot_of(h, tlog)
    tags = tag_of(h)
    dmax = max_dist(window_log)
    for c in range(1, ncell):
        c0, c1 = c * CELL, min(n, (c + 1) * CELL)
        a, b = np.searchsorted(pos, c0), np.searchsorted(pos, c1)
        offs = []
        for i in range(a, b):
            e = int(table[slots[i]])
            p = int(pos[i])
            if (e & 0xFFFFFFFF) != int(tags[i]):
                continue
            s = e >> 32
            d = p - s
            if s >= p or d <= MIN_DIST or d > dmax or d in offs:
                continue
            if not np.array_equal(data[p:p + HASH_BYTES], data[s:s + HASH_BYTES]):
                continue
            offs.append(d)
            if len(offs) == CELL_OFFSETS:
                break
        best = (0, 0, 0)
        for d in offs:
            lo = max(c0, d)
            if lo >= c1:
                continue
            st, ln = longest_run(data[lo:c1] == data[lo - d:c1 - d])
            if ln > best[1]:  # ties: the earlier offset stays
                best = (lo + st, ln, d)
        if best[1] >= min_seg:
            rec[c] = best
    return rec


def partition(n, rec):
    """The frame's blocks in order: ('gap', start, bytes) and ('ldm', start, bytes, distance)."""
    out = []
    ncell = (n + CELL - 1) // CELL
    for c in range(ncell):
        c0, c1 = c * CELL, min(n, (c + 1) * CELL)
        s, ln, d = (int(v) for v in rec[c])
        if ln == 0:
            out.append(("gap", c0, c1 - c0))
            continue
        if s > c0:
            out.append(("gap", c0, s - c0))
        out.append(("ldm", s, ln, d))
        if s + ln < c1:
            out.append(("gap", s + ln, c1 - s - ln))
    return out


# ---- RFC 8878 predefined tables (3.1.1.3.2.2.1-3) and the one-sequence block
NORM_LL = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
NORM_OF = [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]
NORM_ML = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
# match length codes 32..52: (baseline, extra bits)
ML_TABLE = [(35, 1), (37, 1), (39, 1), (41, 1), (43, 2), (47, 2), (51, 3), (59, 3), (67, 4), (83, 4), (99, 5), (131, 7), (259, 8), (515, 9),
            (1027, 10), (2051, 11), (4099, 12), (8195, 13), (16387, 14), (32771, 15), (65539, 16)]


def fse_spread(norm, log):
    size = 1 << log
    table = [None] * size
    high = size - 1
    for s, c in enumerate(norm):
        if c == -1:
            table[high] = s
            high -= 1
    step, mask, pos = (size >> 1) + (size >> 3) + 3, size - 1, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            table[pos] = s
            pos = (pos + step) & mask
            while pos > high:
                pos = (pos + step) & mask
    assert pos == 0 and None not in table
    return table


SPREAD_LL, SPREAD_OF, SPREAD_ML = fse_spread(NORM_LL, 6), fse_spread(NORM_OF, 5), fse_spread(NORM_ML, 6)


def ml_code(ml):
    if ml < 35:
        return ml - 3, 0, 0
    c = max(k for k, (base, _) in enumerate(ML_TABLE) if base <= ml)
    base, bits = ML_TABLE[c]
    assert ml - base < (1 << bits)
    return 32 + c, ml - base, bits


def ldm_block(ml, dist, last):
    """Bytes of the block: empty raw literals, one sequence (LL 0, ML ml, offset value dist + 3)."""
    ofv = dist + 3
    ofc = ofv.bit_length() - 1
    assert ofc <= 28
    mlc, mlx, mln = ml_code(ml)
    acc, nb = 0, 0
    for v, bits in ((mlx, mln), (ofv - (1 << ofc), ofc), (SPREAD_ML.index(mlc), 6), (SPREAD_OF.index(ofc), 5), (SPREAD_LL.index(0), 6), (1, 1)):
        acc |= v << nb
        nb += bits
    stream = acc.to_bytes((nb + 7) // 8, "little")
    body = bytes([0, 1, 0]) + stream
    hdr = (1 if last else 0) | (2 << 1) | (len(body) << 3)
    return hdr.to_bytes(3, "little") + body


def frame_header(n, window_log):
    """Multi-segment header with a 4-byte content size (frames of 64 KiB + 256 B .. 4 GiB)."""
    assert 65536 + 256 <= n <= 0xFFFFFFFF
    return bytes([0x28, 0xB5, 0x2F, 0xFD, 2 << 6, (window_log - 10) << 3]) + n.to_bytes(4, "little")


def model_frame(data, parts, window_log):
    """A frame from a partition: raw blocks for the gaps, one-sequence blocks for the rest."""
    data = np.asarray(data, dtype=np.uint8)
    out = [frame_header(len(data), window_log)]
    for k, part in enumerate(parts):
        last = k + 1 == len(parts)
        if part[0] == "gap":
            _, s, ln = part
            out.append(((1 if last else 0) | (ln << 3)).to_bytes(3, "little"))
            out.append(data[s:s + ln].tobytes())
        else:
            _, s, ln, d = part
            out.append(ldm_block(ln, d, last))
    return b"".join(out)


def saved_bytes(parts):
    """Input bytes the partition hands to one-sequence blocks, and how many such blocks."""
    ldm = [p for p in parts if p[0] == "ldm"]
    return sum(p[2] for p in ldm), len(ldm)

"""Plain-Python model of the decoder's size pass (zh_dec_size_kernel; test infrastructure: pure
Python, no GPU, no libzstd): the bytes a buffer of RFC 8878 frames regenerates, without decoding.

size(buf, dictionary=None) -> (size, ok).  Per buffer, over all its frames (skippable frames skipped):
  * the frame header is parsed as the decoder parses it (reserved bit, window size, Dictionary_ID
    against the dictionary given);
  * the block headers are walked to the last block and the checksum field is skipped: a buffer that
    ends inside a block or before the last block, a reserved block type and a compressed block of
    128 KiB or more are rejected;
  * a frame with a Frame_Content_Size counts that, believed; its block bodies are not looked at;
  * a frame without one is summed per block: Block_Size for raw and RLE blocks; for a compressed
    block the literals' Regenerated_Size plus the sum of the match lengths, read from the sequence
    bitstream with the frame's tables (Repeat_Mode tables carry over from the previous block, a
    formatted dictionary's serve the first), the offsets' extra bits passed over.  Rejected as the
    decoder's sequence reader rejects: no end mark, bits left over at the end, more literal
    lengths than literals, a block total above 128 KiB;
  * the sizes add up in 64 bits, an overflow is rejected; an empty buffer is rejected.
What it cannot see -- an offset that reaches too far, corrupt literal contents, a wrong checksum, a
Frame_Content_Size that lies -- is the decoder's business: for those the model answers a size.

The sequences-section header comes from zh_frames (_sequences), the code tables, the predefined
distributions and the FSE table construction from zh_seqframes; the NCount reader and the backward
bit reader are restated here from RFC 8878 4.1."""
import zh_frames as F
import zh_seqframes as S

BLOCK_MAX = S.BLOCK_MAX
DICT_MAGIC = 0xEC30A437
MAXLOG = (9, 8, 9)  # LL, OF, ML
NSEQ_MAX = BLOCK_MAX // 3 + 2  # (more sequences than this regenerate more than a block may)


class Reject(Exception):
    pass


def _need(ok, why):
    if not ok:
        raise Reject(why)


# ---- FSE table descriptions and tables ----------------------------------------------------------
def read_ncount(p, maxsv, maxlog):
    """FSE table description at p (RFC 8878 4.1.1; bits past the end of p read as zeros) ->
    (normalised counts [maxsv + 1], log, bytes used)."""
    _need(len(p) >= 1, "no table description")
    bits = int.from_bytes(bytes(p), "little")
    log = (bits & 15) + 5
    _need(log <= maxlog, "table log too large")
    pos, rem, thr, nb, norm, prev0 = 4, (1 << log) + 1, 1 << log, log + 1, [], False
    while rem > 1 and len(norm) <= maxsv:
        if prev0:
            n0 = len(norm)
            while True:
                r = (bits >> pos) & 3
                pos += 2
                n0 += r
                if r != 3 or pos >= 8 * len(p) + 32:
                    break
            _need(n0 <= maxsv, "zero run past the last symbol")
            norm += [0] * (n0 - len(norm))
        mx = 2 * thr - 1 - rem
        v = (bits >> pos) & (thr - 1)
        if v < mx:
            pos += nb - 1
        else:
            v = (bits >> pos) & (2 * thr - 1)
            if v >= thr:
                v -= mx
            pos += nb
        c = v - 1
        rem -= abs(c)
        norm.append(c)
        prev0 = c == 0
        while rem < thr:
            nb -= 1
            thr >>= 1
    _need(rem == 1, "counts do not add up")
    used = (pos + 7) // 8
    _need(used <= len(p), "table description runs past its section")
    return norm + [0] * (maxsv + 1 - len(norm)), log, used


class _Tab:
    def __init__(self, cells, log):
        self.cells, self.log = cells, log


def _fse_table(norm, log):
    try:
        return _Tab(S.fse_cells(norm, log), log)
    except AssertionError:
        raise Reject("counts do not fill the table")


_predef = None


def _predefined():
    global _predef
    if _predef is None:
        _predef = [_fse_table(list(n), lg) for n, lg in S.PREDEF]
    return _predef


def _tables(modes, p, prev):
    """The three table descriptions at p (modes: LL, OF, ML as 0..3) -> bytes used; updates prev."""
    o = 0
    for t, m in enumerate(modes):
        if m == 0:
            prev[t] = _predefined()[t]
        elif m == 1:
            _need(o < len(p), "no RLE symbol")
            _need(p[o] <= S.MAXSV[t], "RLE symbol out of range")
            prev[t] = _Tab([(p[o], 0, 0)], 0)
            o += 1
        elif m == 2:
            norm, log, used = read_ncount(p[o:], S.MAXSV[t], MAXLOG[t])
            prev[t] = _fse_table(norm, log)
            o += used
        else:
            _need(prev[t] is not None, "nothing to repeat")
    return o


# ---- the sequence bitstream: lengths only ---------------------------------------------------------
class _Rev:
    """Backward bit reader (RFC 8878 4.1): pos = bits not yet consumed; bits below the stream's
    first read as zeros and drive pos negative."""

    def __init__(self, b):
        _need(len(b) >= 1 and b[-1] != 0, "no end mark")
        self.v = int.from_bytes(bytes(b), "little")
        self.pos = 8 * (len(b) - 1) + b[-1].bit_length() - 1

    def read(self, k):
        lo = self.pos - k
        v = (self.v >> lo) if lo >= 0 else (self.v << -lo)
        self.pos = lo
        return v & ((1 << k) - 1)


def sum_lengths(bits, nseq, tabs):
    """(sum of literal lengths, sum of match lengths) of nseq sequences; tabs = [LL, OF, ML]."""
    r = _Rev(bits)
    st = [r.read(tabs[0].log), r.read(tabs[1].log), r.read(tabs[2].log)]
    sll = sml = 0
    for i in range(nseq):
        ll, of, ml = (tabs[t].cells[st[t]] for t in range(3))
        r.pos -= of[0]  # the offset's extra bits: passed over
        sml += S.ML_BASE[ml[0]] + r.read(S.ML_BITS[ml[0]])
        sll += S.LL_BASE[ll[0]] + r.read(S.LL_BITS[ll[0]])
        if i + 1 < nseq:
            for t, e in ((0, ll), (2, ml), (1, of)):
                st[t] = e[2] + r.read(e[1])
    _need(r.pos <= 0, "bits left over")
    return sll, sml


# ---- blocks and frames ----------------------------------------------------------------------------
def _literals(p):
    """Literals section at the start of block content p -> (section bytes, Regenerated_Size)."""
    _need(len(p) >= 1, "empty block")
    lt, sf = p[0] & 3, (p[0] >> 2) & 3
    if lt <= 1:
        hs = F.RAW_RLE_HDR[sf]
        _need(len(p) >= hs, "literals header runs past the block")
        n = p[0] >> 3 if hs == 1 else int.from_bytes(p[:hs], "little") >> 4
        sec = hs + (n if lt == 0 else 1)
    else:
        hs = 3 if sf <= 1 else sf + 2
        _need(len(p) >= hs, "literals header runs past the block")
        nb = 10 if sf <= 1 else 14 if sf == 2 else 18
        h = int.from_bytes(p[:hs], "little")
        n, cs = (h >> 4) & ((1 << nb) - 1), (h >> (4 + nb)) & ((1 << nb) - 1)
        sec = hs + cs
    _need(n <= BLOCK_MAX and sec <= len(p), "literals section")
    return sec, n


def _compressed_block(p, prev):
    """Regenerated size of compressed block content p; prev = the frame's tables (updated)."""
    sec, nlit = _literals(p)
    s, d = p[sec:], {}
    try:
        F._sequences(s, d)
    except ValueError as e:
        raise Reject(str(e))
    nseq = d["nseq"]
    if nseq == 0:
        return nlit
    _need(nseq <= NSEQ_MAX, "too many sequences")
    o = d["nseq_bytes"]
    m = s[o]
    o += 1
    o += _tables((m >> 6, (m >> 4) & 3, (m >> 2) & 3), s[o:], prev)
    sll, sml = sum_lengths(s[o:], nseq, prev)
    _need(sll <= nlit, "literal lengths exceed the literals")
    _need(nlit + sml <= BLOCK_MAX, "block regenerates more than 128 KiB")
    return nlit + sml


def dict_layout(d):
    """(Dictionary_ID, tables [LL, OF, ML] or None) of a dictionary: formatted (RFC 8878 5) or raw content."""
    d = bytes(d or b"")
    if len(d) < 8 or int.from_bytes(d[:4], "little") != DICT_MAGIC:
        return 0, None
    o = 8
    hb = d[o]
    o += 1 + ((hb - 127 + 1) // 2 if hb >= 128 else hb)  # the Huffman table description
    t = {}
    for k in (1, 2, 0):  # OF, ML, LL
        norm, log, used = read_ncount(d[o:], S.MAXSV[k], MAXLOG[k])
        t[k] = _fse_table(norm, log)
        o += used
    return int.from_bytes(d[4:8], "little"), [t[0], t[1], t[2]]


def _size(b, dictionary):
    _need(len(b) > 0, "empty buffer")
    dict_id, dict_tabs = dict_layout(dictionary) if dictionary else (0, None)
    ip = total = 0
    while ip < len(b):
        n = len(b) - ip
        _need(n >= 4, "magic")
        magic = int.from_bytes(b[ip:ip + 4], "little")
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            _need(n >= 8, "skippable frame header")
            size = 8 + int.from_bytes(b[ip + 4:ip + 8], "little")
            _need(size <= n, "skippable frame runs past the buffer")
            ip += size
            continue
        _need(magic == S.MAGIC and n >= 5, "bad magic")
        fhd = b[ip + 4]
        fcsf, single, chk, didf = fhd >> 6, (fhd >> 5) & 1, (fhd >> 2) & 1, fhd & 3
        _need(not fhd & 8, "reserved bit")
        didn, fcsn = (0, 1, 2, 4)[didf], (single, 2, 4, 8)[fcsf]
        hs = 5 + (0 if single else 1) + didn + fcsn
        _need(n >= hs, "frame header runs past the buffer")
        q = ip + 5
        if not single:
            _need(10 + (b[q] >> 3) <= 30, "window too large")
            q += 1
        did = int.from_bytes(b[q:q + didn], "little")
        q += didn
        fcs = int.from_bytes(b[q:q + fcsn], "little") + (256 if fcsn == 2 else 0) if fcsn else None
        if fcs == (1 << 64) - 1:  # (the decoder's "absent" value: summed instead)
            fcs = None
        _need(did == 0 or (dictionary and did == dict_id), "dictionary mismatch")
        ip += hs
        prev = list(dict_tabs) if dict_tabs else [None, None, None]
        fsize = 0
        while True:
            _need(len(b) - ip >= 3, "block header runs past the buffer")
            bh = int.from_bytes(b[ip:ip + 3], "little")
            last, bt, bsz = bh & 1, (bh >> 1) & 3, bh >> 3
            ip += 3
            _need(bt != 3, "reserved block type")
            _need(bt != 2 or bsz < BLOCK_MAX, "compressed block too large")
            body = 1 if bt == 1 else bsz
            _need(len(b) - ip >= body, "block runs past the buffer")
            if fcs is None:
                fsize += bsz if bt != 2 else _compressed_block(b[ip:ip + bsz], prev)
            ip += body
            if last:
                break
        if chk:
            _need(len(b) - ip >= 4, "checksum runs past the buffer")
            ip += 4
        total += fsize if fcs is None else fcs
        _need(total < 1 << 64, "the sizes overflow 64 bits")
    return total


def size(buf, dictionary=None):
    """-> (size, ok): ok False (size 0) where the size pass reports an error."""
    try:
        return _size(bytes(buf), dictionary), True
    except Reject:
        return 0, False


def drop_content_size(frame):
    """One frame re-framed without its Frame_Content_Size (a window descriptor that covers the
    content in its place, the blocks unchanged), as a streaming writer would have framed it; None
    for a buffer that is not one frame with a content size."""
    b = bytes(frame)
    if len(b) < 6 or int.from_bytes(b[:4], "little") != S.MAGIC:
        return None
    fhd = b[4]
    fcsf, single, didf = fhd >> 6, (fhd >> 5) & 1, fhd & 3
    didn, fcsn = (0, 1, 2, 4)[didf], (single, 2, 4, 8)[fcsf]
    if not fcsn:
        return None
    q = 5 + (0 if single else 1)
    fcs = int.from_bytes(b[q + didn:q + didn + fcsn], "little") + (256 if fcsn == 2 else 0)
    wd = bytes([(max(10, (max(fcs, 1) - 1).bit_length()) - 10) << 3]) if single else b[5:6]
    return b[:4] + bytes([fhd & 0x1F]) + wd + b[q:q + didn] + b[q + didn + fcsn:]


# ---- hand-made buffers whose size is the sum of their parts (the CPU and the GPU test) -----------
FCS_2_40 = 1 << 40


def _asm(buf):
    """Bytes of a zh_seqframes buffer description and the length its frames decode to."""
    want, _, per_frame = S.model(buf)
    assert want is not None
    return S.assemble(buf, per_frame), len(want)


def hand_made():
    """-> [(name, bytes, size, decodable)]: concatenated frames with and without a content size and
    a checksum, skippable frames between them; a frame of raw and RLE blocks only; an 8-byte
    Frame_Content_Size of 2^40 over one raw block (believed: not decodable)."""
    rnd = lambda name, n: S._rng(name).integers(0, 256, n, dtype="uint8").tobytes()  # noqa: E731
    seqs = S.PRE + S.READ
    a = lambda nm: S._block(nm, seqs, 2)  # noqa: E731
    b = lambda nm: S._block(nm, [(4, 5, 1)] * 5, 3, modes=("rle",) * 3)  # noqa: E731
    long = lambda nm: S._block(nm, [(20, 4, 9)] + [(i % 3, 3 + i % 5, 4 + i % 7) for i in range(1, 700)], 5)  # noqa: E731
    two = [S._block("hm_r1", [(4, 5, 6), (9, 9, 9)], 1, modes=(S._fse_norm([4, 9], 6), S._fse_norm([2, 3], 5), S._fse_norm([2, 6], 7))),
           S._block("hm_r2", [(9, 9, 9), (4, 5, 6), (4, 5, 6)], 2, modes=("repeat",) * 3)]
    out = []
    for name, buf in (
        ("two_fcs_nofcs", [S.frame([a("hm_a1")], fcs=True), S.frame([S.raw(b"x"), long("hm_a2")], fcs=False)]),
        ("three_skippable", [S.frame([a("hm_b1")], fcs=True, checksum=True), S.skippable(b"between frames"),
                             S.frame([S.raw(rnd("hm_b2", 300)), b("hm_b3")], fcs=False, checksum=True), S.skippable(b"", nibble=0xF),
                             S.frame(two, fcs=False)]),
        ("four_mixed", [S.skippable(b"first"), S.frame([long("hm_c1")], fcs=False), S.frame([S.rle(7, 100000)], fcs=True),
                        S.skippable(b"z" * 40), S.frame([a("hm_c2"), S.rle(1, 5), b("hm_c3")], fcs=False, checksum=True),
                        S.frame([S.raw(b"tail")], fcs=True, checksum=True)]),
        ("raw_rle_only_nofcs", [S.frame([S.raw(rnd("hm_d1", 1000)), S.rle(0x33, 120000), S.raw(b"q"), S.rle(0, 1)], fcs=False)]),
    ):
        data, n = _asm(buf)
        out.append((name, data, n, True))
    body = rnd("hm_e", 77)
    big = S.MAGIC.to_bytes(4, "little") + bytes([0xE0]) + FCS_2_40.to_bytes(8, "little") + (1 | len(body) << 3).to_bytes(3, "little") + body
    out.append(("fcs_2_40", big, FCS_2_40, False))
    out.append(("fcs_2_40_then_nofcs", big + out[3][1], FCS_2_40 + out[3][2], False))
    return out

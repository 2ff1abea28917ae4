"""Hand-assembled Huffman literals sections (test infrastructure; pure Python and numpy, no GPU,
no libzstd), on top of tests/zh_seqframes.py.

Assembler: huf() describes a Huffman-coded or treeless literals section (RFC 8878 3.1.1.3.1,
4.2) that comp(lits=...) of zh_seqframes accepts besides raw and RLE literals: the bytes, the
weights of symbols 0..last, 1 or 4 streams, a direct or FSE-compressed tree description, a forced
Size_Format, one chosen defect.
Model: the literals are the description's bytes; model_accepts() names what a decoder must reject.
Tracer: segment_trace() restates the segment-parallel stream decode of zh_decode.hip
(huf_streams_par: pass A from guessed entries, Jacobi fix-up rounds, pass B) over one stream and
names the states it went through (tags), so that the vectors' coverage of them is a checked fact.
Vectors: vectors() is the set tests/test_hufframes.py and tests/test_gpu_decode_literals.py decode."""
import numpy as np

import zh_seqframes as S

HUF_LOG_MAX = 11
HP_TRAJ = 32  # trajectory positions pass A records (zh_decode.hip)


# ---- description ------------------------------------------------------------------------------
def huf(data, weights, streams=1, desc="direct", size_format=None, tree=True, damage=None):
    """Huffman literals.  weights: of symbols 0..last, the last non-zero one implied.  desc: "direct"
    or ("fse", norm, log).  size_format None: the smallest legal one.  tree False: a treeless
    section (the weights are the frame's current ones).  damage: one defect (literals_section)."""
    assert streams in (1, 4)
    return {"data": bytes(data), "weights": list(weights), "streams": streams, "desc": desc, "size_format": size_format, "tree": tree,
            "damage": damage}


def code_table(weights):
    """-> (Max_Number_of_Bits, {symbol: (code, bits)}, decode table [(symbol, bits)]): filled as the
    decoder fills it, ascending weight, symbols ascending inside a weight, 2^(w-1) cells each."""
    total = sum((1 << w) >> 1 for w in weights)
    tlog = total.bit_length() - 1
    assert total == 1 << tlog and 1 <= tlog <= HUF_LOG_MAX and weights[-1] > 0, "weights do not fill a table"
    codes, dt, pos = {}, [], 0
    for w in range(1, tlog + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                codes[s] = (pos >> (w - 1), tlog + 1 - w)
                dt += [(s, tlog + 1 - w)] * (1 << (w - 1))
                pos += 1 << (w - 1)
    assert pos == 1 << tlog
    return tlog, codes, dt


def encode_stream(syms, codes, short=False):
    """One stream: the last symbol first, then the final bit flag.  short: the last-decoded
    symbol's code (the first one written) loses its final bit, which must be 0."""
    w = S._Bits()
    for i in range(len(syms) - 1, -1, -1):
        c, k = codes[syms[i]]
        if short and i == len(syms) - 1:
            assert k >= 1 and c & 1 == 0
            c, k = c >> 1, k - 1
        w.add(c, k)
    return w.close()


def weights_desc(weights, desc):
    """The tree description of the explicit weights (all but the last)."""
    ex = weights[:-1]
    nw = len(ex)
    if desc == "direct":
        assert 1 <= nw <= 128
        nib = ex + [0] * (nw & 1)
        return bytes([127 + nw]) + bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(nib), 2))
    _, norm, log = desc
    assert 2 <= nw <= 255 and log <= 6
    cells = S.fse_cells(norm, log)
    tab = S.Table(cells, log)
    # two interleaved states: even-indexed weights from state 1, odd from state 2.  The decoder stops
    # when the update after weight nw-2 overruns the stream, then takes weight nw-1 from the other
    # state: that update must ask for bits
    st = [None, None]
    st[(nw - 1) & 1] = tab.enter(ex[nw - 1], None)[0]
    ends = [u for u, (s, nb, _) in enumerate(cells) if s == ex[nw - 2] and nb > 0]
    assert ends, "no cell of the last-but-one weight reads bits"
    st[(nw - 2) & 1] = ends[0]
    w = S._Bits()
    for i in range(nw - 3, -1, -1):
        st[i & 1], v, k = tab.enter(ex[i], st[i & 1])
        w.add(v, k)
    w.add(st[1], log)
    w.add(st[0], log)
    body = S.ncount_bytes(norm, log, 255) + w.close()
    assert len(body) < 128
    return bytes([len(body)]) + body


def stream_counts(n, streams):
    if streams == 1:
        return [n]
    seg, out = (n + 3) // 4, []
    for _ in range(3):
        out.append(min(seg, n - sum(out)))
    return out + [n - sum(out)]


def literals_section(h, prev):
    """Bytes of the section.  Defects (h["damage"], all rejected by the model):
    ("regen", d): Regenerated_Size off by d; ("zero_front" | "zero_last" | "zero_append" | "short", k):
    stream k with a zero byte in front, its last byte zeroed, a zero byte appended, its last-decoded
    code short of its final 0 bit; "fourth_empty"; ("jump", (s1, s2, s3)): the jump table replaced;
    "boundary": the first stream boundary one byte later; ("desc", bytes): the tree description
    replaced; ("cut", k): the section cut to k bytes."""
    data, weights, ns, dmg = h["data"], h["weights"], h["streams"], h["damage"]
    kind, arg = (dmg if isinstance(dmg, tuple) else (dmg, None))
    n = len(data)
    _, codes, _ = code_table(weights)
    if h["tree"]:
        desc = weights_desc(weights, h["desc"])
        if prev is not None:
            prev[3] = list(weights)
    else:
        desc = b""
        assert prev is None or prev[3] is None or prev[3] == list(weights), "a treeless section is coded with the frame's table"
    if kind == "desc":
        desc = arg
    cnt, streams, at = stream_counts(n, ns), [], 0
    for k, c in enumerate(cnt):
        b = encode_stream(data[at:at + c], codes, short=(kind == "short" and arg == k))
        at += c
        if kind == "zero_front" and arg == k:
            b = b"\x00" + b
        if kind == "zero_last" and arg == k:
            b = b[:-1] + b"\x00"
        if kind == "zero_append" and arg == k:
            b = b + b"\x00"
        streams.append(b)
    if ns == 4:
        jump = [len(b) for b in streams[:3]]
        if kind == "jump":
            jump = list(arg)
        if kind == "boundary":
            jump = [jump[0] + 1, jump[1] - 1, jump[2]]
        if kind == "fourth_empty":
            streams[3] = b""
        body = b"".join(j.to_bytes(2, "little") for j in jump) + b"".join(streams)
    else:
        body = streams[0]
    sec = desc + body
    if kind == "cut":
        sec = sec[:arg]
    nh = n + (arg if kind == "regen" else 0)
    cs = len(sec)
    if ns == 1:
        sf = 0
        assert h["size_format"] in (None, 0)
    else:
        sf = 1 if max(nh, cs) < 1 << 10 else 2 if max(nh, cs) < 1 << 14 else 3
        if h["size_format"] is not None:
            assert h["size_format"] >= sf, "the sizes do not fit the Size_Format"
            sf = h["size_format"]
    nb = (10, 10, 14, 18)[sf]
    assert 0 <= nh < 1 << nb and cs < 1 << nb
    hdr = ((2 if h["tree"] else 3) | sf << 2 | nh << 4 | cs << (4 + nb)).to_bytes((3, 3, 4, 5)[sf], "little")
    h["_sec"] = hdr + sec  # what the assembler emitted (for the tracer)
    return hdr + sec


def model_accepts(h, ctx):
    """Whether a decoder accepts the section; ctx["huf"]: the frame has a Huffman table."""
    n = len(h["data"])
    if h["damage"] is not None:
        return False
    if h["streams"] == 4 and 3 * ((n + 3) // 4) > n:  # no valid split: n = 1, 2, 5
        return False
    if not h["tree"]:
        return ctx["huf"]
    ctx["huf"] = True
    return True


# ---- the decoder's view of an emitted section (from its bytes alone) ------------------------------
def read_ncount(b, max_log):
    """FSE table description (RFC 8878 4.1.1) -> (counts, Accuracy_Log, bytes used), or None."""
    if not b:
        return None
    bits = int.from_bytes(b, "little")
    log = (bits & 15) + 5
    if log > max_log:
        return None
    pos, remaining, threshold, nb, norm, prev0 = 4, (1 << log) + 1, 1 << log, log + 1, [], False
    while remaining > 1 and len(norm) <= 255:
        if prev0:
            while True:
                r = (bits >> pos) & 3
                pos += 2
                norm += [0] * r
                if r != 3 or pos > 8 * len(b) + 32:
                    break
            if len(norm) > 255:
                return None
        mx = 2 * threshold - 1 - remaining
        count = (bits >> pos) & (threshold - 1)
        if count < mx:
            pos += nb - 1
        else:
            count = (bits >> pos) & (2 * threshold - 1)
            if count >= threshold:
                count -= mx
            pos += nb
        count -= 1
        remaining -= abs(count)
        norm.append(count)
        prev0 = count == 0
        while remaining < threshold:
            nb -= 1
            threshold >>= 1
    used = (pos + 7) // 8
    if remaining != 1 or used > len(b):
        return None
    return norm, log, used


def read_weights(p):
    """The tree description at the start of p (RFC 8878 4.2.1) -> (weights of symbols 0..last,
    bytes used), or None where a decoder rejects it."""
    if not p:
        return None
    hb = p[0]
    if hb >= 128:
        nw = hb - 127
        used = 1 + (nw + 1) // 2
        if used > len(p):
            return None
        w = [(p[1 + i // 2] >> (0 if i & 1 else 4)) & 15 for i in range(nw)]
    else:
        used = 1 + hb
        nc = read_ncount(p[1:used], 6) if used <= len(p) else None
        if nc is None:
            return None
        norm, log, k = nc
        try:
            cells = S.fse_cells(norm, log)
        except AssertionError:
            return None
        b = p[1 + k:used]
        if not b or b[-1] == 0:
            return None
        V, pos = int.from_bytes(b, "little"), [8 * (len(b) - 1) + b[-1].bit_length() - 1]

        def rd(k):  # bits below the stream's start read as zeros; pos < 0 afterwards: overrun
            pos[0] -= k
            return (V >> pos[0] if pos[0] >= 0 else V << -pos[0]) & ((1 << k) - 1)

        st, w, i = [rd(log), rd(log)], [], 0
        while True:  # two interleaved states; the stream ends when a state update overruns it
            if len(w) > 253 and i == 0:
                return None
            sym, nb, base = cells[st[i]]
            w.append(sym)
            st[i] = base + rd(nb)
            if pos[0] < 0:
                w.append(cells[st[i ^ 1]][0])
                break
            i ^= 1
    total = sum((1 << x) >> 1 for x in w)
    if max(w) > HUF_LOG_MAX or total == 0:
        return None
    tlog = total.bit_length()
    rest = (1 << tlog) - total
    if tlog > HUF_LOG_MAX or rest & (rest - 1):
        return None
    w.append(rest.bit_length())
    ones = sum(1 for x in w if x == 1)
    if ones < 2 or ones & 1:
        return None
    return w, used


# ---- segment tracer -----------------------------------------------------------------------------
def segment_trace(stream, weights, S_, n):
    """The segment scheme of huf_streams_par over one stream of n symbols cut into S_ segments.
    -> (verdict, tags, symbols): verdict = the counts add up to n and the last exit is bit 0."""
    tags = set()
    tlog, _, dt = code_table(weights)
    if n == 0:
        tags.add("zero_symbols")
    if not stream or stream[-1] == 0:
        return False, tags, None
    V = int.from_bytes(stream, "little")
    top = 8 * (len(stream) - 1) + stream[-1].bit_length() - 1
    Lb = max(-(-top // S_), 1)
    mask = (1 << tlog) - 1
    if Lb >= 65536:
        return False, tags, None
    if Lb == 1:
        tags.add("Lb1")

    def step(p):  # -> (symbol, bits); bits below bit 0 read as zeros
        x = 0 if p <= 0 else (V >> (p - tlog)) & mask if p >= tlog else (V << (tlog - p)) & mask
        return dt[x]

    gA, lo, traj, xA = [], [], [], []
    for j in range(S_):
        hi = top - j * Lb
        if hi <= 0:
            tags.add("empty_segments")
        gA.append(max(hi, 0))
        lo.append(max(top - (j + 1) * Lb, 0))
        p, t = gA[j], []
        while p > lo[j]:
            t.append(p)
            p -= step(p)[1]
        traj.append(t)
        xA.append(p)
    entry, x, c, rounds = list(gA), list(xA), [len(t) for t in traj], 0
    while True:
        px = [top] + x[:-1]
        need = [j for j in range(S_) if entry[j] != px[j]]
        if not need:
            break
        rounds += 1
        assert rounds <= S_ - 1, "lane j is exact after j rounds"
        nx, nc = list(x), list(c)
        for j in need:
            rec = {p: i for i, p in enumerate(traj[j][:HP_TRAJ])}
            late = set(traj[j][HP_TRAJ:])
            p, k, met = px[j], 0, False
            while True:
                if p in rec:
                    nc[j], nx[j] = k + len(traj[j]) - rec[p], xA[j]
                    tags.add("merge_recorded")
                    break
                met = met or p in late
                if p <= lo[j]:
                    nc[j], nx[j] = k, p
                    if met:
                        tags.add("merge_unrecorded")
                    elif k and traj[j]:
                        tags.add("left_segment")
                    break
                p -= step(p)[1]
                k += 1
            entry[j] = px[j]
        x, c = nx, nc
    tags.add("no_fixup" if rounds == 0 else "rounds_max" if rounds == S_ - 1 else "rounds_some")
    if sum(c) != n or x[-1] != 0:
        tags.add("bad_count" if sum(c) != n else "bad_exit")  # (bad_exit: the counts add up, the stream is read past its start)
        return False, tags, None
    out = []
    for j in range(S_):  # pass B
        p = entry[j]
        for _ in range(c[j]):
            if p < tlog:
                tags.add("below_bit0")
            s, k = step(p)
            out.append(s)
            p -= k
    return True, tags, bytes(out)


def section_trace(sec, table):
    """A Huffman or treeless literals section from its bytes (RFC 8878 3.1.1.3.1), its streams through
    segment_trace().  table: the frame's current weights or None.
    -> (verdict, tags, the literals or None, the frame's weights afterwards)."""
    lt, sf = sec[0] & 3, (sec[0] >> 2) & 3
    assert lt >= 2
    hs, nb = (3, 3, 4, 5)[sf], (10, 10, 14, 18)[sf]
    hv = int.from_bytes(sec[:hs], "little")
    n, cs = (hv >> 4) & ((1 << nb) - 1), (hv >> (4 + nb)) & ((1 << nb) - 1)
    no = (False, set(), None, table)
    if hs + cs != len(sec):
        return no
    p = sec[hs:]
    if lt == 2:
        r = read_weights(p)
        if r is None:
            return no
        table, p = r[0], p[r[1]:]
    elif table is None:
        return no
    no = (False, set(), None, table)
    if sf == 0:
        parts = [(p, n)]
    else:
        if len(p) < 10:
            return no
        s = [int.from_bytes(p[2 * i:2 * i + 2], "little") for i in range(3)]
        seg = (n + 3) // 4
        if 6 + sum(s) >= len(p) or 3 * seg > n:
            return no
        parts, at = [], 6
        for k in range(4):
            sz = s[k] if k < 3 else len(p) - at
            parts.append((p[at:at + sz], seg if k < 3 else n - 3 * seg))
            at += sz
    ok, tags, got = True, set(), b""
    for b, c in parts:
        v, t, syms = segment_trace(b, table, 64 // len(parts), c)
        ok = ok and v
        tags |= t
        got += syms or b""
    return ok, tags, got if ok else None, table


_traces = {}


def vector_trace(v):
    """The tracer over every Huffman / treeless section of a vector, the table state kept per frame.
    -> (verdict, {streams: tags}), computed once; asserts that accepted sections decode to their
    description's bytes."""
    if v.name + v.form in _traces:
        return _traces[v.name + v.form]
    ok, tags = True, {1: set(), 4: set()}
    for f in v.buf:
        table = None
        for b in f.get("blocks", ()):
            if b["type"] == "comp" and isinstance(b["lits"], dict):
                h = b["lits"]
                good, t, got, table = section_trace(h["_sec"], table)
                tags[h["streams"]] |= t
                if good:
                    assert got == h["data"], (v, "the tracer decodes other bytes")
                    if h["tree"]:
                        assert table == h["weights"], (v, "the description reads back as other weights")
                ok = ok and good
    _traces[v.name + v.form] = (ok, tags)
    return ok, tags


# ---- the vectors ------------------------------------------------------------------------------
TWO_SYMS = [1, 1]  # Max_Number_of_Bits 1; direct, header byte 128
FIXED7 = [1] * 128  # 127 explicit weights (an odd count: the padding nibble), a 7-bit fixed code
FIXED8_256 = [1] * 256  # 255 FSE-compressed weights, the most a description holds
FIXED8_255 = [1] * 254 + [2]  # 254: the other state ends the weight stream
FSE_ONES = ("fse", [0, 31, 1], 5)
SKEW11 = [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 1]  # lengths 1..11
EVEN = [3, 3, 3, 1, 1, 1, 1]  # lengths 2, 2, 2, 4, 4, 4, 4: a wrong-parity entry never resynchronises
SLOW_SYNC = [4, 4, 4, 2, 2, 2, 1, 1]  # lengths 2, 2, 2, 4, 4, 4, 5, 5: only symbols 6, 7 change the parity
DIRECT_EVEN = [2, 1, 1]  # a direct description with an even count of explicit weights
# lengths 2, 2, 2, 4, 4, 4, 5, 6..11, 11: SLOW_SYNC's parity trap with long codes to stretch segments
SLOW_LONG = [10, 10, 10, 8, 8, 8, 7, 6, 5, 4, 3, 2, 1, 1]
# non-zero weights only at the ends of the table build's four 64-symbol lane groups: lengths 2, 2, 3,
# 4, 5, 6, 6, 2; ties (weights 5 and 1) and single classes, across groups
SPREAD = [0] * 256
for _s, _w in ((0, 5), (63, 5), (64, 4), (127, 3), (128, 2), (191, 1), (192, 1), (255, 5)):
    SPREAD[_s] = _w
SPREAD_SYMS = [s for s, w in enumerate(SPREAD) if w]
FSE_SPREAD = ("fse", [57, 2, 1, 1, 1, 2], 6)

TAGS = ("rounds_max", "merge_recorded", "merge_unrecorded", "left_segment", "no_fixup", "Lb1", "empty_segments", "below_bit0", "zero_symbols")


def _uni(name, n, k):
    return S._rng(name).integers(0, k, n, dtype=np.uint8).tobytes()


def _slow(name, n, period=150):
    """Uniform over the even-length symbols 0..5, the odd-length symbol 6 at every period-th place."""
    a = S._rng(name).integers(0, 6, n, dtype=np.uint8)
    a[period - 1::period] = 6
    return a.tobytes()


def _slow_long(name, n, at, run):
    """11-bit symbols (12, 13) around a run of _slow() data: few symbols, long segments."""
    a = S._rng(name).integers(12, 14, n, dtype=np.uint8)
    a[at:at + run] = np.frombuffer(_slow(name + "r", run, 60), np.uint8)
    return a.tobytes()


def _skew(name, n, bits=None):
    """Symbols of SKEW11 drawn towards the long codes; bits: the most the stream may hold."""
    r = S._rng(name)
    a = r.integers(4, 12, n, dtype=np.uint8)
    length = lambda s: min(int(s) + 1, 11)  # noqa: E731
    if bits is not None:
        total = sum(length(s) for s in a)
        while total > bits:
            i = int(r.integers(0, n))
            total -= length(a[i]) - 1
            a[i] = 0
    return a.tobytes()


def _direct_bytes(ex):
    nib = list(ex) + [0] * (len(ex) & 1)
    return bytes([127 + len(ex)]) + bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(nib), 2))


def _descriptions():
    """-> list of (name, forms, builder, expect, opts); builder(pre, kw) -> the buffer (zh_seqframes).
    opts["walk"]: per Huffman / treeless block (literals type, header bytes, streams, weight kind)."""
    D = []

    def add_buf(name, fn, forms, walk, expect=0, **opts):
        D.append((name, forms, fn, expect, dict(opts, walk=walk)))

    def add(name, mk, hdr, seqs=(), forms="Q", expect=0, **opts):
        """mk() -> a fresh description; the block is the frame's only one (Q) or follows a raw block (S)."""
        h = mk()
        walk = [("huffman" if h["tree"] else "treeless", hdr, h["streams"], ("direct" if h["desc"] == "direct" else "fse") if h["tree"] else None)]
        add_buf(name, lambda pre, kw: [S.frame(([S.raw(S.PRE_RAW)] if pre else []) + [S.comp(mk(), list(seqs))], **kw)], forms, walk, expect,
                **opts)

    H1 = lambda *a, **k: (lambda: huf(*a, **k))  # noqa: E731
    # -- one stream (64 segments)
    for n in list(range(10)) + [63, 64, 65]:  # every padding-bit position; one-bit and empty segments; no symbols
        add(f"two_syms_{n}", H1(_uni(f"two{n}", n, 2), TWO_SYMS), 3)
    add("fixed7_1000", H1(_uni("f7a", 1000, 128), FIXED7), 3, align16=True)  # 63 fix-up rounds
    add("fixed7_1023", H1(_uni("f7b", 1023, 128), FIXED7), 3)  # 7,161 bits: 64 segments of 112, no fix-up
    add("skew11_1023", H1(_skew("sk1023", 1023, 8 * 1016 - 2), SKEW11), 3)  # Compressed_Size near its 10 bits' end
    add("even_1s", H1(_uni("even1", 1000, 7), EVEN), 3)
    add("slow_long_1s", H1(_slow_long("sl_900_100_330_60", 900, 100, 330), SLOW_LONG), 3)  # (found with the tracer: a merge past the recorded trajectory)
    add("direct_even_1s", H1(_uni("de1", 301, 3), DIRECT_EVEN), 3)
    add("fixed8_256_1s", H1(_uni("f8a", 900, 256), FIXED8_256, desc=FSE_ONES), 3)
    add("fixed8_255_1s", H1(bytes(x % 255 for x in _uni("f8b", 777, 256)), FIXED8_255, desc=FSE_ONES), 3)
    add("spread_1s", H1(bytes(SPREAD_SYMS[x] for x in _uni("sp1", 1001, 8)), SPREAD, desc=FSE_SPREAD), 3)
    # -- four streams (16 segments each)
    for n in (3, 4, 6, 7, 8, 9):  # 9: the fourth stream is the single byte 01
        add(f"two_syms_4s_{n}", H1(_uni(f"two4{n}", n, 2), TWO_SYMS, 4), 3, libzstd_may_reject=n < 6)
    add("skew11_4s_1021", H1(_skew("sk1021", 1021, 8 * 990), SKEW11, 4), 3, align16=True)
    add("fixed7_4s_1022", H1(_uni("f7_1022", 1022, 128), FIXED7, 4), 3)
    add("even_4s_1023", H1(_uni("even1023", 1023, 7), EVEN, 4), 3, align16=True)
    add("slow_4s_1024", H1(_slow("slow1024", 1024), SLOW_SYNC, 4), 4)
    add("slow_4s_16383", H1(_slow("slow16383", 16383), SLOW_SYNC, 4), 4)
    add("slow_4s_16384", H1(_slow("slow16384", 16384), SLOW_SYNC, 4), 5)
    add("two_syms_4s_131072", H1(_uni("two128k", 131072, 2), TWO_SYMS, 4), 5)  # a whole block of literals, no sequences
    add("fixed7_4s_rmax", H1(_uni("f7r", 2001, 128), FIXED7, 4), 4, align16=True)
    add("fixed8_256_4s_rmax", H1(_uni("f8r", 3001, 256), FIXED8_256, 4, desc=FSE_ONES), 4)
    add("even_4s_rmax", H1(_uni("evenr", 2999, 7), EVEN, 4), 4)
    add("slow_4s_3000", H1(_slow("slow3000", 3000), SLOW_SYNC, 4), 4)
    add("spread_4s", H1(bytes(SPREAD_SYMS[x] for x in _uni("sp4", 2003, 8)), SPREAD, 4, desc=FSE_SPREAD), 4)
    add("fixed8_255_4s", H1(bytes(x % 255 for x in _uni("f8c", 1500, 256)), FIXED8_255, 4, desc=FSE_ONES), 4)
    add("forced_sf3", H1(_skew("sf3", 101), SKEW11, 4, size_format=3), 5)
    add("forced_sf2", H1(_skew("sf2", 102), SKEW11, 4, size_format=2), 4)
    # -- with sequences: literal runs end around the stream boundaries k * seg and at every dword phase
    n4 = 3999  # seg = 1000
    lls = [997, 5, 999, 1001, 3, 990]  # runs end at 997, 1002, 2001, 3002, 3005, 3995; 4 trail
    seq4 = [(ll, (40, 4, 7, 66, 3, 5)[i], (3 + 3, 20 + 3, 1 + 3, 2, 1, 9 + 3)[i]) for i, ll in enumerate(lls)]
    add("skew11_4s_seqs", H1(_skew("sk4s", n4), SKEW11, 4), 4, seq4, forms="QS")
    seq1 = [(7, 5, 2 + 3), (61, 4, 30 + 3), (2, 33, 1), (130, 3, 2), (0, 6, 3), (90, 70, 4 + 3)]  # 290 of 301 literals
    add("skew11_1s_seqs", H1(_skew("sk1s", 301), SKEW11), 3, seq1, forms="QS")

    # -- treeless sections: the frame's table outlives raw and RLE literals and is replaced by a new tree
    def five(pre, kw):
        fse3 = (S._fse_norm([4, 9], 6), S._fse_norm([2, 3], 5), S._fse_norm([2, 6], 7))
        return [S.frame([S.comp(huf(_skew("t5a", 500), SKEW11, 4), [(100, 5, 6), (3, 40, 5)]),
                         S._block("t5b", [(4, 5, 6), (9, 9, 9)], 1, modes=fse3),
                         S.comp(huf(_skew("t5c", 1203), SKEW11, 4, tree=False), [(1000, 9, 1), (200, 4, 44)]),
                         S.comp(("rle", 0x33, 40), [(30, 6, 2)]),
                         S.comp(huf(_skew("t5e", 333), SKEW11, 1, tree=False), [])], **kw)]

    add_buf("treeless_five_blocks", five, "S", [("huffman", 3, 4, "direct"), ("treeless", 4, 4, None), ("treeless", 3, 1, None)])

    def second_tree(pre, kw):
        return [S.frame([S.comp(huf(_skew("t2a", 200), SKEW11, 1), [(10, 5, 6)]),
                         S.comp(huf(_uni("t2b", 400, 7), EVEN, 4), []),
                         S.comp(huf(_uni("t2c", 900, 7), EVEN, 4, tree=False), [(100, 5, 6)]),
                         S.comp(huf(_uni("t2d", 90, 7), EVEN, 1, tree=False), [])], **kw)]

    add_buf("treeless_second_tree", second_tree, "S", [("huffman", 3, 1, "direct"), ("huffman", 3, 4, "direct"), ("treeless", 3, 4, None),
                                                      ("treeless", 3, 1, None)])
    # -- rejects (no content size, no checksum: only the defect can be what a decoder rejects)
    C = S.CORRUPT
    bad = lambda name, mk, hdr: add(name, mk, hdr, expect=C, variant=1)  # noqa: E731
    d1 = _skew("rej1", 200)
    bad("regen_plus1", H1(d1, SKEW11, damage=("regen", 1)), 3)
    bad("regen_minus1", H1(d1, SKEW11, damage=("regen", -1)), 3)
    bad("zero_front", H1(d1, SKEW11, damage=("zero_front", 0)), 3)
    bad("zero_last", H1(d1, SKEW11, damage=("zero_last", 0)), 3)
    bad("zero_append", H1(d1, SKEW11, damage=("zero_append", 0)), 3)
    # the code of the last-decoded symbol short of its final 0 bit: zero fill finds the symbol, the
    # stream is consumed past its start (a decoder that clamps the position at 0 accepts this)
    bad("short_code", H1(d1[:-1] + b"\x0a", SKEW11, damage=("short", 0)), 3)
    d4 = _skew("rej4", 1501)
    bad("fourth_empty", H1(d4, SKEW11, 4, damage="fourth_empty"), 4)
    bad("jump_past", H1(d4, SKEW11, 4, damage=("jump", (0xFFFF, 3, 3))), 4)
    bad("boundary_moved", H1(d4, SKEW11, 4, damage="boundary"), 4)
    bad("regen4_minus1", H1(d4, SKEW11, 4, damage=("regen", -1)), 4)
    bad("regen4_plus3", H1(d4, SKEW11, 4, damage=("regen", 3)), 4)
    bad("zero_front_4s", H1(d4, SKEW11, 4, damage=("zero_front", 2)), 4)
    bad("short_code_4s", H1(d4[:-1] + b"\x0a", SKEW11, 4, damage=("short", 3)), 4)
    for n in (1, 2, 5):
        bad(f"no_split_{n}", H1(_uni(f"ns{n}", n, 2), TWO_SYMS, 4), 3)
    dw = _uni("rejw", 100, 2)
    for name, ex in (("weight_12", [12, 1, 1]), ("max_bits_12", [11, 11]), ("weights_all_zero", [0, 0, 0]), ("weights_not_pow2", [3, 3, 1]),
                     # (an odd count of weight-1 symbols cannot be written: were the count of ones odd the
                     # sum would be odd, the remainder then 1 and the implied weight the even-making
                     # one; the same check's other arm, fewer than two ones, is reachable)
                     ("weights_no_ones", [2])):
        bad(name, H1(dw, TWO_SYMS, damage=("desc", _direct_bytes(ex))), 3)
    bad("desc_past_section", H1(dw, FIXED7, damage=("cut", 40)), 3)
    fse_desc = weights_desc(SPREAD, FSE_SPREAD)
    nc = len(S.ncount_bytes(FSE_SPREAD[1], FSE_SPREAD[2], 255))
    assert nc >= 3
    bad("fse_desc_truncated", lambda: huf(bytes(SPREAD_SYMS[x] for x in _uni("rejf", 100, 8)), SPREAD, desc=FSE_SPREAD,
                                          damage=("desc", bytes([nc - 2]) + fse_desc[1:nc - 1])), 3)
    add("treeless_first_block", H1(d1, SKEW11, tree=False), 3, expect=C, variant=1)
    add_buf("treeless_second_frame", lambda pre, kw: [S.frame([S.comp(huf(d1, SKEW11), [])], **kw), S.frame([S.comp(huf(d1, SKEW11, tree=False), [])], **kw)],
            "S", [("huffman", 3, 1, "direct"), ("treeless", 3, 1, None)], expect=C, variant=1)
    # -- a valid section, one byte of capacity missing
    add("cap_short_4s", H1(_skew("short", 777), SKEW11, 4), 3, expect=S.TOO_SMALL, short=True, variant=0)
    return D


REJECTED = {"regen_plus1", "regen_minus1", "zero_front", "zero_last", "zero_append", "short_code", "fourth_empty", "jump_past", "boundary_moved",
            "regen4_minus1", "regen4_plus3", "zero_front_4s", "short_code_4s", "no_split_1", "no_split_2", "no_split_5", "weight_12", "max_bits_12",
            "weights_all_zero", "weights_not_pow2", "weights_no_ones", "desc_past_section", "fse_desc_truncated", "treeless_first_block",
            "treeless_second_frame"}

_cache = {}


def vectors():
    """Every literal vector (built once), as zh_seqframes.Vector."""
    if "v" not in _cache:
        V = []
        for idx, (name, forms, fn, expect, opts) in enumerate(_descriptions()):
            kw = S._frame_kw(opts.get("variant", idx), expect)
            for form in forms:
                V.append(S.Vector(name, form, fn(1 if form == "S" else 0, kw), expect, **opts))
        _cache["v"] = V
    return _cache["v"]


def huf_blocks(v):
    """The Huffman descriptions of a vector's blocks, in order."""
    return [b["lits"] for f in v.buf for b in f.get("blocks", ()) if b["type"] == "comp" and isinstance(b["lits"], dict)]


def without_content_size(v):
    """The vector's buffer framed without Frame_Content_Size."""
    import copy

    buf = copy.deepcopy(v.buf)
    for f in buf:
        f["fcs"] = False
    return S.assemble(buf, S.model(buf)[2])

"""Hand-assembled RFC 8878 frames with chosen sequences (test infrastructure; pure Python and
numpy, no GPU, no libzstd).

Assembler: a buffer is a list of frames and skippable frames; a frame a list of blocks (raw, RLE,
compressed with raw or RLE literals); a compressed block a literal string and explicit
(literal_length, match_length, Offset_Value) triples, Offset_Value being the coded value (1-3 the
repeat codes, else offset + 3), with each of the three sequence tables predefined, RLE,
FSE-described from given normalised counts, or repeated from the frame's previous block.
Model: a plain executor of the same description (RFC 8878 3.1.1.4-5) that returns the bytes, or
None where a decoder must reject, and names the semantic cases it met (tags).
Vectors: vectors() / dict_vectors() build the set the tests decode, each block once as the
buffer's only block (form Q: the decoder's quad sequence kernel and 2 KiB execution window) and
once after a 1-byte raw block (form S: its serial reader and 8 KiB window)."""
import bisect
import copy
import ctypes
import zlib

import numpy as np

import zh_testlib as T

BLOCK_MAX = 128 * 1024
MAGIC = 0xFD2FB528

# sequence codes (RFC 8878 3.1.1.3.2.1.1): baselines and extra bits
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
# predefined distributions (RFC 8878 3.1.1.3.2.2.1-3): table logs 6, 5, 6
LL_NORM = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
OF_NORM = [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]
ML_NORM = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
PREDEF = ((LL_NORM, 6), (OF_NORM, 5), (ML_NORM, 6))  # table order: LL, OF, ML
MAXSV = (35, 31, 52)


def ll_code(v):
    return bisect.bisect_right(LL_BASE, v) - 1


def ml_code(v):
    return bisect.bisect_right(ML_BASE, v) - 1


def of_code(ofv):
    return ofv.bit_length() - 1


def fse_cells(norm, log):
    """FSE decoding table of normalised counts: cells (symbol, bits, baseline)."""
    size = 1 << log
    sym, nxt, high = [0] * size, [], size - 1
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
        nxt.append(1 if c == -1 else c)
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    assert pos == 0, "counts do not fill the table"
    cells = []
    for u in range(size):
        ns = nxt[sym[u]]
        nxt[sym[u]] += 1
        nb = log - (ns.bit_length() - 1)
        cells.append((sym[u], nb, (ns << nb) - size))
    return cells


class Table:
    def __init__(self, cells, log):
        self.log, self.by_sym = log, {}
        for u, (s, nb, base) in enumerate(cells):
            self.by_sym.setdefault(s, []).append((base, nb, u))

    def enter(self, sym, nxt):
        """The cell of `sym` from which the decoder reaches state `nxt` (None: any): cell, bits, count."""
        assert sym in self.by_sym, f"symbol {sym} is not in the table"
        for base, nb, u in self.by_sym[sym]:
            if nxt is None:
                return u, 0, 0
            if base <= nxt < base + (1 << nb):
                return u, nxt - base, nb
        raise AssertionError("no cell reaches the state")


_predef = None


def predefined_tables():
    global _predef
    if _predef is None:
        _predef = [Table(fse_cells(n, lg), lg) for n, lg in PREDEF]
    return _predef


class _Bits:
    """Forward bit writer (the decoder reads the stream from its end)."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def add(self, v, k):
        assert 0 <= v < (1 << k) or (k == 0 and v == 0)
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def close(self):
        self.add(1, 1)
        if self.n:
            self.out.append(self.acc)
        return bytes(self.out)


def ncount_bytes(norm, log, maxsv):
    """FSE table description of normalised counts (the oracle's writer)."""
    last = max(s for s, c in enumerate(norm) if c)
    a = np.zeros(256, np.int16)
    a[:len(norm)] = norm
    out = np.zeros(512, np.uint8)
    n = T.oracle().orc_fse_write_ncount(out.ctypes.data_as(T.vp), ctypes.c_size_t(512), a.ctypes.data_as(T.vp), ctypes.c_uint32(last),
                                        ctypes.c_uint32(log))
    assert 0 < n < 512 and last <= maxsv
    return out[:n].tobytes()


def xxh64(b):
    a = np.frombuffer(bytes(b), np.uint8).copy() if len(b) else np.zeros(1, np.uint8)
    return int(T.oracle().orc_xxh64(a.ctypes.data, len(b)))


# ---- description ------------------------------------------------------------------------------
def raw(data):
    return {"type": "raw", "data": bytes(data)}


def rle(byte, n):
    return {"type": "rle", "byte": byte, "n": n}


def comp(lits, seqs, modes=("predefined",) * 3, surplus=False, zero_last=False):
    """Compressed block.  lits: bytes (raw literals), ("rle", byte, n) or a Huffman description
    (zh_hufframes.huf).  modes (LL, OF, ML): "predefined", "rle", ("fse", counts, log) or "repeat".
    surplus / zero_last damage the bitstream (rejects)."""
    return {"type": "comp", "lits": lits, "seqs": [tuple(s) for s in seqs], "modes": tuple(modes), "surplus": surplus, "zero_last": zero_last}


def frame(blocks, fcs=True, checksum=False, dict_id=0):
    """fcs: single segment with the content size; else a window descriptor and no content size."""
    return {"blocks": list(blocks), "fcs": fcs, "checksum": checksum, "dict_id": dict_id}


def skippable(data, nibble=3):
    return {"skip": bytes(data), "nibble": nibble}


def _lits_len(lits):
    if isinstance(lits, dict):
        return len(lits["data"])
    return lits[2] if isinstance(lits, tuple) else len(lits)


# ---- assembler --------------------------------------------------------------------------------
def _literals_section(lits, prev=None):
    """prev: the frame's current tables; prev[3] = the weights of its Huffman table (updated)."""
    if isinstance(lits, dict):
        import zh_hufframes as H

        return H.literals_section(lits, prev)
    t, n = (1, lits[2]) if isinstance(lits, tuple) else (0, len(lits))
    body = bytes([lits[1]]) if t else bytes(lits)
    if n < 32:
        return bytes([t | n << 3]) + body
    if n < 4096:
        return (t | 1 << 2 | n << 4).to_bytes(2, "little") + body
    assert n < 1 << 20
    return (t | 3 << 2 | n << 4).to_bytes(3, "little") + body


def _sequences_section(b, prev):
    """prev: the frame's current tables [LL, OF, ML] (updated)."""
    seqs = b["seqs"]
    n = len(seqs)
    if n == 0:
        return b"\x00"
    hdr = bytes([n]) if n < 128 else bytes([(n >> 8) + 128, n & 255]) if n < 0x7F00 else b"\xff" + (n - 0x7F00).to_bytes(2, "little")
    codes = []
    for ll, ml, ofv in seqs:
        lc, mc, oc = ll_code(ll), ml_code(ml), of_code(ofv)
        codes.append(((lc, ll - LL_BASE[lc], LL_BITS[lc]), (oc, ofv - (1 << oc), oc), (mc, ml - ML_BASE[mc], ML_BITS[mc])))
    mbyte, desc = 0, b""
    for t, mode in enumerate(b["modes"]):
        if mode == "predefined":
            m, prev[t] = 0, predefined_tables()[t]
        elif mode == "rle":
            s = codes[0][t][0]
            assert all(c[t][0] == s for c in codes), "an RLE table needs one code"
            m, prev[t] = 1, Table([(s, 0, 0)], 0)
            desc += bytes([s])
        elif mode == "repeat":
            assert prev[t] is not None, "nothing to repeat"
            m = 3
        else:
            _, norm, log = mode
            m, prev[t] = 2, Table(fse_cells(norm, log), log)
            desc += ncount_bytes(norm, log, MAXSV[t])
        mbyte |= m << (6 - 2 * t)
    # written back to front: the decoder reads, per sequence, the extra bits OF, ML, LL, then the
    # state updates LL, ML, OF (none after the last), after the initial states LL, OF, ML
    w, st = _Bits(), [None, None, None]
    for i in range(n - 1, -1, -1):
        upd = []
        for t in range(3):
            st[t], v, k = prev[t].enter(codes[i][t][0], st[t])
            upd.append((v, k))
        if i != n - 1:
            for t in (1, 2, 0):
                w.add(*upd[t])
        for t in (0, 2, 1):
            w.add(codes[i][t][1], codes[i][t][2])
    for t in (2, 1, 0):
        w.add(st[t], prev[t].log)
    bits = w.close()
    if b["surplus"]:
        bits = b"\x00" + bits
    if b["zero_last"]:
        bits = bits[:-1] + b"\x00"
    return hdr + bytes([mbyte]) + desc + bits


def _block_bytes(b, last, prev):
    if b["type"] == "raw":
        body, t, size = b["data"], 0, len(b["data"])
    elif b["type"] == "rle":
        body, t, size = bytes([b["byte"]]), 1, b["n"]
    else:
        body = _literals_section(b["lits"], prev) + _sequences_section(b, prev)
        t, size = 2, len(body)
        assert size < BLOCK_MAX, "compressed block too large"
    assert size < 1 << 21
    return (int(last) | t << 1 | size << 3).to_bytes(3, "little") + body


def assemble(buf, content=None):
    """Bytes of a buffer description.  content: the model's bytes per frame (content sizes and
    checksums; None where the model rejects: the declared size is then what the blocks claim)."""
    out, k = b"", 0
    for f in buf:
        if "skip" in f:
            out += (0x184D2A50 | f["nibble"]).to_bytes(4, "little") + len(f["skip"]).to_bytes(4, "little") + f["skip"]
            continue
        body = content[k] if content is not None and content[k] is not None else None
        k += 1
        size = len(body) if body is not None else _claimed_size(f)
        did = f["dict_id"]
        didf = 0 if did == 0 else 1 if did < 256 else 2 if did < 65536 else 3
        if f["fcs"]:
            fcsf = 0 if size < 256 else 1 if size < 65536 + 256 else 2
            fhd = fcsf << 6 | 1 << 5
            tail = (size - 256 if fcsf == 1 else size).to_bytes((1, 2, 4)[fcsf], "little")
        else:
            wlog = max(10, (max(size, 1) - 1).bit_length())
            fhd, tail = 0, b""
        hdr = bytes([fhd | int(f["checksum"]) << 2 | didf]) + (b"" if f["fcs"] else bytes([(wlog - 10) << 3]))
        hdr += did.to_bytes((0, 1, 2, 4)[didf], "little") + tail
        out += MAGIC.to_bytes(4, "little") + hdr
        prev = [None, None, None, None]  # LL, OF, ML tables; the Huffman table's weights
        for i, b in enumerate(f["blocks"]):
            out += _block_bytes(b, i == len(f["blocks"]) - 1, prev)
        if f["checksum"]:
            out += (xxh64(body if body is not None else b"") & 0xFFFFFFFF).to_bytes(4, "little")
    return out


def lenient_bytes(buf):
    """The bytes of a buffer that has one defect, the defect ignored: what a lenient decoder returns."""
    clean = copy.deepcopy(buf)
    for f in clean:
        for b in f.get("blocks", ()):
            if b["type"] == "comp":
                b["surplus"] = False
    out = []
    for f in clean:
        if "blocks" in f:
            r = model([f], limit=1 << 30)[0]
            assert r is not None
            out.append(r)
    return b"".join(out)


def _claimed_size(f):
    n = 0
    for b in f["blocks"]:
        n += len(b["data"]) if b["type"] == "raw" else b["n"] if b["type"] == "rle" else _lits_len(b["lits"]) + sum(s[1] for s in b["seqs"])
    return n


# ---- model ------------------------------------------------------------------------------------
EXEC_WINDOWS = (2048, 8192)  # the decoder's two execution windows


def _edge_tags(tags, kind, p):
    for W in EXEC_WINDOWS:
        for e, nm in ((W - 1, "m1"), (W, "0"), (W + 1, "p1"), (2 * W, "2w")):
            if p == e:
                tags.add(f"W{W}_{kind}_{nm}")


def _run_block(b, out, pos, hist0, rep, tags, ctx, limit=BLOCK_MAX):
    """Executes compressed block b into out at pos; hist0 = bytes before out[0] (dictionary).
    Returns the new pos, or None to reject."""
    lits = b["lits"]
    nlit = _lits_len(lits)
    seqs = b["seqs"]
    n = len(seqs)
    if b["surplus"] or b["zero_last"]:
        return None
    if isinstance(lits, dict):  # Huffman literals: the bytes are the description's data
        import zh_hufframes as H

        if not H.model_accepts(lits, ctx):
            return None
    if sum(s[0] for s in seqs) > nlit or nlit + sum(s[1] for s in seqs) > limit:
        return None
    if isinstance(lits, dict):
        L = np.frombuffer(lits["data"], np.uint8)
        tags.add(f"lit_huf{lits['streams']}" if lits["tree"] else f"lit_treeless{lits['streams']}")
    else:
        L = np.full(nlit, lits[1], np.uint8) if isinstance(lits, tuple) else np.frombuffer(lits, np.uint8)
        tags.add("lit_rle" if isinstance(lits, tuple) else "lit_raw")
    for t, nm in enumerate(("ll", "of", "ml")):
        m = b["modes"][t]
        tags.add(f"{nm}_{m if isinstance(m, str) else 'fse'}")
    for cnt in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 0x7EFF, 0x7F00):
        if n == cnt:
            tags.add(f"nseq_{cnt}")
    trail = nlit - sum(s[0] for s in seqs)
    if n:
        tags.add("trailing_literals" if trail else "no_trailing_literals")
        if n % 64 == 0:
            tags.add("nseq_mult64_trailing" if trail else "nseq_mult64_no_trailing")
    modes = b["modes"]
    if n and modes == ("rle",) * 3 and LL_BITS[ll_code(seqs[0][0])] == 0 and ML_BITS[ml_code(seqs[0][1])] == 0 and seqs[0][2] == 1:
        tags.add("tables_all_rle_empty_bitstream")
    if n and modes == ("repeat",) * 3:
        tags.add("repeat_after_" + ctx["last_modes"])
    if n and "repeat" not in modes:
        kinds = {m if isinstance(m, str) else "fse" for m in modes}
        ctx["last_modes"] = kinds.pop() if len(kinds) == 1 else "mixed"
    maxlogs = all(not isinstance(m, str) and m[2] == lg for m, lg in zip(modes, (9, 8, 9)))
    b0, lp, chain = pos, 0, {1: 0, 3: 0}
    for i, (ll, ml, ofv) in enumerate(seqs):
        lc, mc, oc = ll_code(ll), ml_code(ml), of_code(ofv)
        for nm, c, v, base, bits in (("ll", lc, ll, LL_BASE, LL_BITS), ("ml", mc, ml, ML_BASE, ML_BITS)):
            if bits[c]:
                if v == base[c]:
                    tags.add(f"{nm}_code{c}_lo")
                if v == base[c] + (1 << bits[c]) - 1:
                    tags.add(f"{nm}_code{c}_hi")
        if ofv == 1 << oc:
            tags.add(f"of_code{oc}_lo")
        if ofv == (2 << oc) - 1:
            tags.add(f"of_code{oc}_hi")
        if maxlogs and LL_BITS[lc] == 16 and ML_BITS[mc] >= 15 and oc >= 16:
            tags.add("maxbits_" + ("first" if i == 0 else "last" if i == n - 1 else "mid"))
        # literals
        if ll:
            _edge_tags(tags, "lstart", pos - b0)
            _edge_tags(tags, "lend", pos - b0 + ll)
        out[pos:pos + ll] = L[lp:lp + ll]
        lp += ll
        pos += ll
        # offset and repeat history (RFC 8878 3.1.1.5)
        first = i == 0 and ctx["first_seq"]
        if ofv > 3:
            off = ofv - 3
            for k in range(3):
                if off == rep[k]:
                    tags.add(f"explicit_equals_rep{k}")
            rep[:] = [off, rep[0], rep[1]]
        else:
            name = f"rep{ofv}_" + ("ll0" if ll == 0 else "ll")
            tags.add(name)
            if first:
                tags.add(("frame2_" if ctx["frame"] else "") + "first_" + name)
            if i == 0 and ctx["comp_blocks"]:
                tags.add("rep_from_previous_block")
                for g in ctx["between"]:
                    tags.add("rep_past_" + g + "_block")
            idx = ofv - 1 + (1 if ll == 0 else 0)
            if idx == 0:
                off = rep[0]
            else:
                off = rep[0] - 1 if idx == 3 else rep[idx]
                if off == 0:  # libzstd: a zero offset is forced to 1
                    off = 1
                    tags.add("rep3_ll0_forced_to_1")
                if idx == 1:
                    rep[:] = [off, rep[0], rep[2]]
                else:
                    rep[:] = [off, rep[0], rep[1]]
        if off > pos + len(hist0):
            return None
        # match
        s = pos - off
        _edge_tags(tags, "mstart", pos - b0)
        _edge_tags(tags, "mend", pos - b0 + ml)
        if ml > off:
            tags.add("overlap")
            if ml > 65536 and off & (off - 1):
                tags.add("overlap_long_odd_period")
            if ll + ml == BLOCK_MAX and n == 1:
                tags.add(f"fill_off{off}")
        for W in EXEC_WINDOWS:
            ms, ws = pos - b0, (pos - b0) // W * W
            if (ms + ml - 1) // W - ms // W >= 2:
                if ms - off >= ws:
                    tags.add(f"W{W}_span3_source_inside")
                if ms - off + min(off, ml) <= ws:
                    tags.add(f"W{W}_span3_source_before")
            if ms - off < ws < ms - off + min(off, ml) and ws > 0:
                tags.add(f"W{W}_source_straddles_start")
        if ll == 0 and ml == 3 and off in chain:
            chain[off] += 1
            if chain[off] >= 64:
                tags.add(f"chain64_off{off}")
        else:
            chain = {1: 0, 3: 0}
        if s < 0:
            tags.add("dict_match_runs_into_frame" if s + ml > 0 else "dict_match_inside")
            if ml > off:
                tags.add("dict_overlap_off_gt_pos")
            k = min(ml, -s)
            out[pos:pos + k] = hist0[len(hist0) + s:len(hist0) + s + k]
            pos, s, ml = pos + k, s + k, ml - k
        if ml <= off:
            out[pos:pos + ml] = out[s:s + ml]
        else:  # overlapping: the last `off` bytes repeat
            out[pos:pos + ml] = np.resize(out[s:pos].copy(), ml)
        pos += ml
    out[pos:pos + trail] = L[lp:]
    if trail:
        _edge_tags(tags, "lstart", pos - b0)
    ctx["first_seq"] = ctx["first_seq"] and n == 0
    return pos + trail


def model(buf, dictionary=b"", limit=BLOCK_MAX):
    """-> (bytes or None, tags, per-frame bytes).  None: a decoder must reject the buffer.
    limit: the most a block may regenerate (RFC 8878 3.1.1.2.4: 128 KiB)."""
    tags, frames, ok = set(), [], True
    hist0 = np.frombuffer(bytes(dictionary), np.uint8)
    nf = 0
    for f in buf:
        if "skip" in f:
            tags.add("skippable")
            continue
        tags.add("content_size" if f["fcs"] else "no_content_size")
        if f["checksum"]:
            tags.add("checksum")
        if f["dict_id"]:
            tags.add("dict_id")
        out = np.zeros(_claimed_size(f) + 8, np.uint8)
        pos, rep = 0, [1, 4, 8]
        ctx = {"first_seq": True, "frame": nf, "comp_blocks": 0, "between": [], "last_modes": None, "huf": False}
        nf += 1
        for b in f["blocks"]:
            if b["type"] == "raw":
                out[pos:pos + len(b["data"])] = np.frombuffer(b["data"], np.uint8)
                pos += len(b["data"])
                ctx["between"].append("raw")
            elif b["type"] == "rle":
                out[pos:pos + b["n"]] = b["byte"]
                pos += b["n"]
                ctx["between"].append("rle")
            else:
                pos = _run_block(b, out, pos, hist0, rep, tags, ctx, limit)
                if pos is None:
                    break
                if b["seqs"]:
                    ctx["comp_blocks"] += 1
                    ctx["between"] = []
        if pos is None:
            ok = False
            frames.append(None)
            break
        frames.append(out[:pos].tobytes())
    return (b"".join(frames) if ok else None), tags, frames


# ---- the vectors ------------------------------------------------------------------------------
OVERLAP_OFFSETS = list(range(1, 17)) + [17, 31, 33, 63, 64, 65, 127, 255, 1000, 2047, 2048, 2049, 8191, 8192, 8193]
SEQ_COUNTS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129)

_E = [f"W{W}_{k}_{e}" for W in EXEC_WINDOWS for k in ("lstart", "lend", "mstart", "mend") for e in ("m1", "0", "p1", "2w")]
ALL_SEQ_PATHS = set(
    ["rep1_ll", "rep2_ll", "rep3_ll", "rep1_ll0", "rep2_ll0", "rep3_ll0", "first_rep1_ll", "first_rep2_ll", "first_rep3_ll",
     "rep3_ll0_forced_to_1", "explicit_equals_rep0", "explicit_equals_rep1", "explicit_equals_rep2", "overlap", "overlap_long_odd_period",
     "chain64_off1", "chain64_off3", "trailing_literals", "no_trailing_literals", "nseq_mult64_trailing", "nseq_mult64_no_trailing",
     "maxbits_first", "maxbits_mid", "maxbits_last", "tables_all_rle_empty_bitstream", "lit_raw", "lit_rle", "skippable", "checksum",
     "content_size", "no_content_size", "nseq_32511", "nseq_32512"]
    + [f"{t}_{m}" for t in ("ll", "of", "ml") for m in ("predefined", "rle", "fse")]
    + [f"fill_off{o}" for o in OVERLAP_OFFSETS] + [f"nseq_{n}" for n in SEQ_COUNTS] + _E
    + [f"W{W}_{k}" for W in EXEC_WINDOWS for k in ("span3_source_inside", "span3_source_before", "source_straddles_start")]
    # LL code 35 and ML code 52 at their upper ends regenerate more than a block may hold
    + [f"ll_code{c}_{e}" for c in range(16, 36) for e in ("lo", "hi") if (c, e) != (35, "hi")]
    + [f"ml_code{c}_{e}" for c in range(32, 53) for e in ("lo", "hi") if (c, e) != (52, "hi")]
    # OF code 17's upper end (offset 262,140) is out of a lone block's reach: DICT_SEQ_PATHS
    + [f"of_code{c}_{e}" for c in range(0, 18) for e in ("lo", "hi") if (c, e) != (17, "hi")])
# a second compressed block, a second frame or megabytes of history: never a buffer's only block
S_ONLY_SEQ_PATHS = set(["rep_from_previous_block", "rep_past_raw_block", "rep_past_rle_block", "frame2_first_rep2_ll", "first_rep3_ll0",
                        "repeat_after_predefined", "repeat_after_rle", "repeat_after_fse", "ll_repeat", "of_repeat", "ml_repeat"]
                       + ["of_code17_hi"] + [f"of_code{c}_{e}" for c in range(18, 23) for e in ("lo", "hi")])
DICT_SEQ_PATHS = {"first_rep1_ll0", "first_rep2_ll0", "first_rep3_ll0", "dict_match_inside", "dict_match_runs_into_frame", "dict_overlap_off_gt_pos", "of_code16_hi", "of_code17_lo", "of_code17_hi"}

CORRUPT, TOO_SMALL = 6, 7
LIT_RAW_MAX = 120000  # raw literals up to here leave room for the sequences in a block below 128 KiB


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _block(name, seqs, trail=0, modes=("predefined",) * 3, lits=None, **kw):
    n = sum(s[0] for s in seqs) + trail
    if lits is None:
        lits = _rng(name).integers(0, 256, n, dtype=np.uint8).tobytes() if n <= LIT_RAW_MAX else ("rle", 0x5A, n)
    return comp(lits, seqs, modes, **kw)


def _segs(segs):
    """("L", n) / ("M", n, offset) runs -> sequences with explicit offsets, trailing literals."""
    seqs, ll = [], 0
    for s in segs:
        if s[0] == "L":
            ll += s[1]
        else:
            seqs.append((ll, s[1], s[2] + 3))
            ll = 0
    return seqs, ll


PRE = [(40, 5, 13), (3, 4, 26), (2, 6, 20)]  # leaves the repeat history 17, 23, 10
READ = [(3, 4, 1), (3, 4, 2), (3, 4, 3), (2, 5, 1)]  # reads the history back out
PRE_RAW = b"\xa5"  # form S: the raw block in front


def _fse_norm(syms, log):
    """Counts of one cell for each of syms, the rest on a symbol not among them."""
    norm = [0] * (max(max(syms), 3) + 1)
    for s in syms:
        norm[s] = 1
    spare = next(s for s in range(4) if s not in syms)
    norm[spare] = (1 << log) - len(syms)
    return ("fse", norm, log)


def _maxbits_modes():
    return (_fse_norm([1, 35], 9), _fse_norm([2, 16], 8), _fse_norm([0, 51], 9))


def _descriptions():
    """-> list of (name, forms, builder, expect, opts).  builder(pre, kw) -> the buffer: pre = bytes in
    front of the block (form S: 1), kw = the frame header's options."""
    D = []

    def add(name, fn, forms="QS", expect=0, **opts):
        """fn(pre) -> the blocks that follow the raw block of form S in one frame."""
        add_buf(name, lambda pre, kw: [frame(([raw(PRE_RAW)] if pre else []) + fn(pre), **kw)], forms, expect, **opts)

    def add_buf(name, fn, forms, expect=0, **opts):
        D.append((name, forms, fn, expect, opts))

    one = lambda name, seqs, trail=0, **kw: (lambda pre: [_block(name, seqs, trail, **kw)])  # noqa: E731
    # -- repeat offsets
    cases = [(5, 7, k) for k in (1, 2, 3)] + [(0, 7, k) for k in (1, 2, 3)] + [(4, 5, o + 3) for o in (17, 23, 10)]
    add("rep_cases", one("rep_cases", [s for c in cases for s in PRE + [c] + READ], 3))  # each from the history 17, 23, 10
    for k in (1, 2, 3):
        add(f"first_rep{k}", one(f"first_rep{k}", [(12, 5, k)] + READ, 2))
    add("rep3_ll0_forced", one("rep3_ll0_forced", [(5, 3, 1), (0, 4, 3)] + READ, 2))
    add("first_rep3_ll0", one("first_rep3_ll0", [(0, 4, 3)] + READ, 2), forms="S")
    add("history_across_blocks", lambda pre: [_block("hab1", PRE, 4), raw(_rng("hab2").integers(0, 256, 20, dtype=np.uint8).tobytes()),
                                              rle(0x77, 30), _block("hab3", [(3, 5, 1), (0, 4, 1), (2, 4, 3)] + READ, 2)], forms="S")
    add_buf("history_reset_frame2", lambda pre, kw: [frame([_block("hr1", PRE, 3)], **kw), frame([_block("hr2", [(12, 5, 2)] + READ, 2)], **kw)], "S")
    add_buf("skippable_first", lambda pre, kw: [skippable(b"metadata!"),
                                                frame(([raw(PRE_RAW)] if pre else []) + [_block("skippable_first", PRE + READ, 2)], **kw)], "QS")
    # -- overlap and the period arithmetic
    for o in OVERLAP_OFFSETS:
        add(f"fill_off{o}", one(f"fill_off{o}", [(o, BLOCK_MAX - o, o + 3)]))
    chain = [(8193, 3, 4)]
    for o in OVERLAP_OFFSETS:
        chain += [(2, ml, o + 3) for ml in (3, o - 1, o, o + 1, 63, 64, 65) if ml >= 3]
    add("overlap_chain", one("overlap_chain", chain, 5))
    # -- window edges
    for d, nm in ((-1, "m1"), (0, "0"), (1, "p1")):
        a, b, c, ca, cb, cc = [], [], [], 0, 0, 0
        for p in (2048 + d, 4096, 8192 + d, 16384):  # W + d and 2 W of both windows
            a += [("L", p - ca), ("M", 40, 9)]  # a match starts at p after literals
            b += [("L", p - 40 - cb), ("M", 40, 11)]  # a match ends at p, literals follow
            c += [("L", p - 40 - cc), ("M", 40, 13), ("M", 30, 47)]  # two matches meet at p
            ca, cb, cc = p + 40, p, p + 30
        add(f"edge_start_{nm}", one(f"edge_start_{nm}", _segs(a)[0], 6))
        add(f"edge_end_{nm}", one(f"edge_end_{nm}", _segs(b + [("L", 9), ("M", 5, 3)])[0], 0))
        add(f"edge_meet_{nm}", one(f"edge_meet_{nm}", _segs(c)[0], 4))
    for W in EXEC_WINDOWS:
        add(f"W{W}_span3_inside", one(f"W{W}_span3_inside", _segs([("L", W + 100), ("M", 2 * W + 500, 37)])[0], 7))
        add(f"W{W}_span3_before", one(f"W{W}_span3_before", _segs([("L", 3 * W + 100), ("M", 2 * W + 500, 3 * W + 50)])[0], 0))
        add(f"W{W}_straddle", one(f"W{W}_straddle", _segs([("L", W + 20), ("M", 100, 60), ("L", 3), ("M", 70, 100)])[0], 1))
    for o in (3, 1):
        add(f"chain_off{o}", one(f"chain_off{o}", [(10, 3, o + 3)] + [(0, 3, o + 3)] * 150, 3))
    # -- sequence counts
    # (trailing literals: none after odd counts, 5 after even ones, and 64 and 128 both ways)
    for n, trail in [(n, 5 * (1 - n % 2)) for n in SEQ_COUNTS] + [(64, 0), (128, 0)]:
        seqs = [(20, 4, 9)] + [(i % 3, 3 + i % 5, (4 + i % 7) if i % 4 else 1 + i % 3) for i in range(1, n)]
        add(f"nseq_{n}_t{trail}", one(f"nseq_{n}_t{trail}", seqs, trail))
    for n in (0x7EFF, 0x7F00):
        add(f"nseq_{n}", one(f"nseq_{n}", [(4, 3, 6)] + [(0, 3, 4 + i % 4) for i in range(1, n)], n & 1))
    # -- length and offset codes at both ends
    llv = [v for c in range(16, 36) for v in (LL_BASE[c], LL_BASE[c] + (1 << LL_BITS[c]) - 1)][:-1]
    mlv = [v for c in range(32, 53) for v in (ML_BASE[c], ML_BASE[c] + (1 << ML_BITS[c]) - 1)][:-1]
    for nm, vals, mk in (("ll", llv, lambda v: (v, 3, 5)), ("ml", mlv, lambda v: (1, v, 8))):
        groups = []
        for v in sorted(vals, reverse=True):  # first fit, largest first
            g = next((g for g in groups if sum(g) + v + 8 * len(g) <= LIT_RAW_MAX), None)
            if g is None:
                groups.append([v])
            else:
                g.append(v)
        for k, g in enumerate(groups):
            seqs = [mk(v) for v in g]
            if nm == "ml":
                seqs[0] = (8,) + seqs[0][1:]
            add(f"{nm}_codes_{k}", one(f"{nm}_codes_{k}", seqs, 2))
    ofs, pos = [(9, 3, 1), (2, 3, 2), (2, 3, 3)], 21
    for c in range(2, 17):
        for ofv in ((1 << c), (2 << c) - 1)[:1 if c == 16 else 2]:
            ll = max(ofv - 3 - pos, 0) + 1
            ofs.append((ll, 3, ofv))
            pos += ll + 3
    add("of_codes_low", one("of_codes_low", ofs, 1))
    # (more literals than a raw section holds in one block: RLE literals, which show an offset's
    # reach but not its bytes; dict_vectors() has both offsets over random bytes)
    add("of_code16_hi", one("of_code16_hi", [(131068, 4, 131071)]))
    add("of_code17_lo", one("of_code17_lo", [(131069, 3, 131072)]))
    add_buf("of_codes_high", lambda pre, kw: [frame(_high_offset_frame(), **kw)], "S")  # megabytes of history
    # -- the most bits a step of a first block can take, first / mid-stream / last
    short, big = (1, 3, 4), (65536, 32771 + 0x5555, 65537)
    for nm, seqs in (("first", [big] + [short] * 8), ("mid", [short] * 4 + [big] + [short] * 4), ("last", [short] * 8 + [big])):
        add(f"maxbits_{nm}", one(f"maxbits_{nm}", seqs, 0, modes=_maxbits_modes()), align16=True)
    # -- table shapes
    add("tables_all_rle", one("tables_all_rle", [(4, 5, 1)] * 5, 3, modes=("rle",) * 3))
    add("tables_mixed", one("tables_mixed", [(17, 9, 5), (40, 9, 6), (2, 9, 4)], 1, modes=(_fse_norm([2, 16, 23], 6), "rle", "predefined")))
    rseqs = [(4, 5, 6), (4, 5, 5)]
    fse3 = (_fse_norm([4, 9], 6), _fse_norm([2, 3], 5), _fse_norm([2, 6], 7))
    for nm, modes, sq in (("predefined", ("predefined",) * 3, rseqs), ("rle", ("rle",) * 3, rseqs), ("fse", fse3, [(4, 5, 6), (9, 9, 9)])):
        two = [_block("ra_" + nm, sq, 1, modes=modes), _block("rb_" + nm, sq[::-1] + sq, 2, modes=("repeat",) * 3)]
        add(f"repeat_after_{nm}", (lambda two: lambda pre: two)(two), forms="S")
    # -- rejects (the model returns None)
    add("bad_offset_first", lambda pre: [_block("bad_offset_first", [(6, 4, 6 + pre + 1 + 3)], 2)], expect=CORRUPT)
    add("bad_offset_later_block", lambda pre: [raw(b"0123456789"), _block("bad_offset_later", [(3, 4, 10 + pre + 3 + 1 + 3)], 2)], forms="S",
        expect=CORRUPT)
    add("ll_exceeds_literals", one("ll_exceeds_literals", [(5, 4, 4), (6, 3, 5)], lits=b"0123456789"), expect=CORRUPT)
    add("regen_131073", one("regen_131073", [(10, 131063, 6)]), expect=CORRUPT, libzstd_lenient=True)
    add("surplus_byte", one("surplus_byte", PRE + READ, 2, surplus=True), expect=CORRUPT, libzstd_lenient=True)
    add("last_byte_zero", one("last_byte_zero", PRE + READ, 2, zero_last=True), expect=CORRUPT)
    add("cap_short_fcs", one("cap_short", PRE + READ, 2), expect=TOO_SMALL, short=True, variant=0)
    add("cap_short_nofcs", one("cap_short", PRE + READ, 2), expect=TOO_SMALL, short=True, variant=1)
    return D


def _high_offset_frame():
    """OF codes 17-22 at both ends: the history is RLE blocks (4 bytes of input per 128 KiB), with
    64 random bytes in a raw block around each match source so that an offset one byte out shows."""
    H = (1 << 23) + 4096
    seqs, pos = [], H
    for c in range(17, 23):
        for ofv in (1 << c, (2 << c) - 1):
            seqs.append((1, 8, ofv))
            pos += 9
    spans, p = [], H
    for ll, ml, ofv in seqs:
        s = p + ll - (ofv - 3)
        spans.append((s - 16, s + 48))
        p += ll + ml
    spans.sort()
    merged = []
    for a, b in spans:
        if merged and a <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], b)
        else:
            merged.append([a, b])
    blocks, cur, r, k = [], 0, _rng("of_codes_high"), 0
    for a, b in merged + [[H, H]]:
        while cur < a:
            n = min(a - cur, BLOCK_MAX)
            blocks.append(rle(0x10 + k % 200, n))
            k += 1
            cur += n
        if b > a:
            blocks.append(raw(r.integers(0, 256, b - a, dtype=np.uint8).tobytes()))
            cur = b
    return blocks + [_block("of_codes_high", seqs, 1)]


class Vector:
    def __init__(self, name, form, buf, expect, dictionary=None, **opts):
        self.name, self.form, self.buf, self.expect, self.dictionary, self.opts = name, form, buf, expect, dictionary, opts
        self.want, self.tags, per_frame = model(buf, dictionary or b"")
        self.bytes = assemble(buf, per_frame)
        self.align16 = opts.get("align16", False)
        # what libzstd may return instead of an error where versions differ (None: an error only)
        self.libzstd_may_return = None
        if opts.get("libzstd_lenient"):
            self.libzstd_may_return = lenient_bytes(buf)
        if opts.get("short"):  # a valid frame, one byte of capacity missing
            self.cap = len(self.want) - 1
        else:
            self.cap = len(self.want) if self.want is not None else sum(_claimed_size(f) for f in buf if "blocks" in f) + 16
        assert (self.want is None) == (expect == CORRUPT), name

    def __repr__(self):
        return f"{self.name}/{self.form}"


def _frame_kw(variant, expect=0):
    """Frame header options in rotation.  A vector that must be rejected carries no checksum, so
    that only its defect can be what a decoder rejects."""
    return {"fcs": variant % 2 == 0, "checksum": variant % 4 >= 2 and expect != CORRUPT}


_cache = {}


def vectors():
    """Every vector without a dictionary (built once)."""
    if "v" in _cache:
        return _cache["v"]
    V = []
    for idx, (name, forms, fn, expect, opts) in enumerate(_descriptions()):
        kw = _frame_kw(opts.get("variant", idx), expect)
        for form in forms:
            V.append(Vector(name, form, fn(1 if form == "S" else 0, kw), expect, **opts))
    V.append(Vector("dict_id_without_dictionary", "Q", [frame([_block("did", PRE + READ, 2)], dict_id=0x1234)], "nonzero"))
    _cache["v"] = V
    return V


def dictionary():
    return _rng("dictionary").integers(0, 256, BLOCK_MAX, dtype=np.uint8).tobytes()


def dict_vectors():
    """Vectors that need the raw-content dictionary() in front of the frame."""
    if "d" in _cache:
        return _cache["d"]
    d, n, V = dictionary(), BLOCK_MAX, []
    cases = [("dict_inside", lambda pre: [(5, 20, 5 + pre + 1000 + 3)] + READ, 2, 0),
             ("dict_into_frame", lambda pre: [(10, 40, 10 + pre + 15 + 3)] + READ, 2, 0),
             ("dict_overlap", lambda pre: [(4, 100, 4 + pre + 6 + 3)] + READ, 2, 0),
             # a frame's first sequence without literals: the initial history 1, 4, 8 reaches the dictionary
             ("dict_first_rep1_ll0", lambda pre: [(0, 5, 1)] + READ, 2, 0),
             ("dict_first_rep2_ll0", lambda pre: [(0, 5, 2)] + READ, 2, 0),
             ("dict_first_rep3_ll0", lambda pre: [(0, 5, 3)] + READ, 2, 0),
             ("dict_bad_offset", lambda pre: [(6, 4, n + 6 + pre + 1 + 3)], 2, CORRUPT),  # (not the batch's first or last output)
             ("dict_of_code16_hi", lambda pre: [(10 - pre, 3, 131071)], 2, 0),
             ("dict_of_code17_lo", lambda pre: [(5 - pre, 3, 131072)], 2, 0),
             ("dict_of_code17_hi", lambda pre: [(131068 - pre, 4, 262143)], 0, 0)]
    for idx, (name, fn, trail, expect) in enumerate(cases):
        for form in "QS":
            pre = 1 if form == "S" else 0
            blocks = ([raw(PRE_RAW)] if pre else []) + [_block(name, fn(pre), trail)]
            V.append(Vector(name, form, [frame(blocks, **_frame_kw(idx, expect))], expect, dictionary=d))
    _cache["d"] = V
    return V

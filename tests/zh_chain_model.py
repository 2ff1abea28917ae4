"""A plain restatement of the encoder's FSE chain kernel (zh_entropy.hip k3_chain, "K3") and of
the packing kernel's ("K4") indexing of its output (test infrastructure; pure Python plus the
oracle's exported stages).

For an input of at most 64 KiB (one block, level 3) the model takes the oracle's parse
(orc_lz_parse, offsets resolved against the repcodes 1, 4, 8), computes the LL / OF / ML codes,
picks each table's mode as select_encoding_type does and builds its CTable as build_ctable does
(oracle/zstd_oracle.c), then runs each table's chain twice:

  serial     the state before every encoding step e, from init_state of the last sequence's
             code: exactly the kernel's init_state / step lambdas, with the min(..., 1023) clamp
             and the dead steps (e == 0 or e >= nbSeq) that pass the state through;
  segmented  as k3_chain runs it: L = ZH_K3_SEGLEN(nbSeq), 21 segments; the entry guess of
             segment g > 0 is stT[0] run through the last min(L / 16, 8) batches of segment
             g - 1; a first pass over every segment; then Jacobi rounds with entry(g) =
             exit(g - 1), in which a re-run compares its state with the stored one at the first
             step of each 16-step batch only, returns "merged" there and leaves the exit as it
             was.  The final state is the exit of segment 20.

trace() asserts that the segmented scheme stored exactly the serial chain's states and final
state (a census from a wrong model is worth nothing) and names the states the scheme went
through as tags (TAGS).  A merge at batch 0 cannot happen: a segment is re-run because its entry
differs from the stored first state, which is what batch 0 compares.  It has no tag.

zh_k3_magic / zh_k3_index (zh_common.h) are restated too: k3_magic, k3_index."""
import ctypes

import numpy as np

import zh_frames as F
import zh_testlib as T

# zh_common.h / zh_entropy.hip
SEGS, SLOTS, RUN, BATCH, WARM, SEQ_CAP = 21, 64, 16, 16, 128, 13120
SW_BITS = 184 * 32  # the bit sink's LDS words (SW_WORDS): what one K4 append must fit
CLAMP = 1023
TABLES = ("ll", "of", "ml")

# RFC 8878 §3.1.1.3.2.1: extra bits per code, predefined distributions
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEF = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
ML_DEF = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
OF_DEF = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
# per table: max symbol, largest table log, predefined (norm, log, max symbol)
SHAPE = {"ll": (35, 9, LL_DEF, 6, 35), "of": (31, 8, OF_DEF, 5, 28), "ml": (52, 9, ML_DEF, 6, 52)}

TAGS = ("no_fixup", "rounds_max", "rounds_max_l64", "ran_to_end", "merge_mid", "merge_last", "rerun_twice", "dead_tail", "short_warmup",
        "full_warmup", "clamped")


def seglen(nbseq):
    """ZH_K3_SEGLEN"""
    return ((nbseq + SEGS - 1) // SEGS + RUN - 1) & ~(RUN - 1)


def k3_bytes(nbseq):
    """ZH_K3_BYTES"""
    return 3 * SLOTS * seglen(nbseq)


def k3_magic(L):
    return ((1 << 24) + L - 1) // L


def k3_index(e, t, L, m):
    """zh_k3_index, 32-bit arithmetic as the device does it"""
    g = (((e << 8) & 0xFFFFFFFF) * m) >> 32
    r = (e - g * L) & 0xFFFFFFFF
    return (((r // RUN) * SLOTS + 3 * g + t) * RUN + (r & (RUN - 1))) & 0xFFFFFFFF


def ll_code(ll):
    if ll > 63:
        return ll.bit_length() + 18
    return ll if ll < 16 else (16, 16, 17, 17, 18, 18, 19, 19)[ll - 16] if ll < 24 else 20 if ll < 28 else 21 if ll < 32 else 22 if ll < 40 else 23 if ll < 48 else 24


def ml_code(mlb):
    if mlb > 127:
        return mlb.bit_length() + 35
    if mlb < 32:
        return mlb
    return 32 + (mlb - 32) // 2 if mlb < 40 else 36 + (mlb - 40) // 4 if mlb < 48 else 38 + (mlb - 48) // 8 if mlb < 64 else 40 if mlb < 80 else 41 if mlb < 96 else 42


class _CTable(ctypes.Structure):
    class Sym(ctypes.Structure):
        _fields_ = [("dFS", ctypes.c_int), ("dNb", ctypes.c_uint32)]

    _fields_ = [("log", ctypes.c_uint32), ("st", ctypes.c_uint16 * 4096), ("sym", Sym * 256)]


def parse(data):
    """The oracle's level-3 sequences of one block: [(ll, ml, off)] and their Offset_Values."""
    O = T.oracle()
    d = np.ascontiguousarray(data, dtype=np.uint8)
    assert 0 < len(d) <= 65536
    seq = np.zeros((len(d) // 5 + 2, 3), np.uint32)
    last = ctypes.c_uint32(0)
    ns = O.orc_lz_parse(d.ctypes.data_as(T.vp), ctypes.c_uint32(len(d)), seq.ctypes.data_as(T.vp), ctypes.byref(last))
    rep = (ctypes.c_uint32 * 3)(1, 4, 8)
    ofb = np.zeros(ns + 1, np.uint32)
    O.orc_resolve_repcodes(seq.ctypes.data_as(T.vp), ctypes.c_size_t(ns), rep, ofb.ctypes.data_as(T.vp))
    return seq[:ns].tolist(), ofb[:ns].tolist()


def build_table(name, codes):
    """(mode, log, stT, dNb, dFS) of one table for the codes in sequence order: select_encoding_type
    and build_ctable of the oracle."""
    O = T.oracle()
    max_sym, fse_log, def_norm, def_log, def_max = SHAPE[name]
    n = len(codes)
    count = [0] * (max_sym + 1)
    for c in codes:
        count[c] += 1
    mx = max(s for s in range(max_sym + 1) if count[s])
    most = max(count)
    allowed = mx <= 28 if name == "of" else True
    if most == n:
        mode = "predefined" if allowed and n <= 2 else "rle"
    elif allowed and (n < (1 << def_log) or most < (n >> (def_log - 1))):
        mode = "predefined"
    else:
        mode = "fse"
    if mode == "rle":  # FSE_buildCTable_rle: one state, no bits
        dnb, dfs = [0] * (max_sym + 1), [0] * (max_sym + 1)
        return mode, 0, [0, 0], dnb, dfs
    ct = _CTable()
    if mode == "predefined":
        norm, log, top = np.array(def_norm, np.int16), def_log, def_max
    else:
        log = int(O.orc_fse_optimal_table_log(ctypes.c_uint32(fse_log), ctypes.c_size_t(n), ctypes.c_uint32(mx)))
        cnt, n1 = np.array(count, np.uint32), n
        if cnt[codes[-1]] > 1:
            cnt[codes[-1]] -= 1
            n1 -= 1
        norm, top = np.zeros(64, np.int16), mx
        r = O.orc_fse_normalize(norm.ctypes.data_as(T.vp), ctypes.c_uint32(log), cnt.ctypes.data_as(T.vp), ctypes.c_size_t(n1), ctypes.c_uint32(mx),
                                ctypes.c_int(n1 >= 2048))
        assert r == log, (name, r, log)
    assert O.orc_fse_build_ctable(ctypes.byref(ct), norm.ctypes.data_as(T.vp), ctypes.c_uint32(top), ctypes.c_uint32(log)) == 0
    st = list(ct.st[:1 << log])
    # a symbol above the table's largest is never coded; the kernel's dead steps use code 0
    dnb = [ct.sym[s].dNb if s <= top else 0 for s in range(max_sym + 1)]
    dfs = [ct.sym[s].dFS if s <= top else 0 for s in range(max_sym + 1)]
    return mode, log, st, dnb, dfs


class Chain:
    """One table's chain: codes in encoding order (step e codes sequence nbSeq - 1 - e), padded
    with code 0 to 21 L steps as K2 lays them out."""

    def __init__(self, name, codes, fixup=True, jacobi_entry=True):
        self.name, self.n = name, len(codes)
        self.mode, self.log, self.st, self.dnb, self.dfs = build_table(name, codes)
        self.L = seglen(self.n)
        self.nk = self.L // BATCH
        self.codes = list(reversed(codes)) + [0] * (SEGS * self.L - self.n)
        self.clamped = False
        self.fixup, self.jacobi_entry = fixup, jacobi_entry  # (switched off only by the mutation check)

    def init_state(self, code):
        d = self.dnb[code]
        nb = ((d + (1 << 15)) & 0xFFFFFFFF) >> 16
        return self.st[((((nb << 16) - d) & 0xFFFFFFFF) >> nb) + self.dfs[code]]

    def step(self, s, e):
        """the state after step e from state s (a dead step passes s through)"""
        if e < 1 or e >= self.n:
            return s
        c = self.codes[e]
        nb = ((s + self.dnb[c]) & 0xFFFFFFFF) >> 16
        i = ((s >> nb) + self.dfs[c]) & 0xFFFFFFFF
        if i > CLAMP:
            self.clamped = True
            i = CLAMP
        return self.st[i]

    def bits(self, s, e):
        """state bits step e (live) writes from state s"""
        return ((s + self.dnb[self.codes[e]]) & 0xFFFFFFFF) >> 16

    def serial(self):
        """state before every step e < 21 L, and the final state"""
        s = self.init_state(self.codes[0])
        out = []
        for e in range(SEGS * self.L):
            out.append(s)
            s = self.step(s, e)
        return out, s

    def segmented(self):
        """-> stored states, final state, rounds, events [(round, segment, merged batch or None)]"""
        L, nk = self.L, self.nk
        store = [None] * (SEGS * L)
        entry, x = [0] * SEGS, [0] * SEGS
        for g in range(SEGS):
            if g == 0:
                s = self.init_state(self.codes[0])
            else:
                s = self.st[0]
                for k in range(max(nk - WARM // BATCH, 0), nk):
                    for q in range(BATCH):
                        s = self.step(s, (g - 1) * L + BATCH * k + q)
            entry[g] = s
            x[g] = self._pass(g, s, store, False)[0]
        rounds, events = 0, []
        while self.fixup:
            ne = [entry[g] if g == 0 else (x[g - 1] if self.jacobi_entry else entry[g]) for g in range(SEGS)]
            active = [g for g in range(SEGS) if ne[g] != entry[g]]
            if not active:
                break
            rounds += 1
            assert rounds <= SEGS - 1, "segment g is exact after round g"
            for g in active:
                entry[g] = ne[g]
                s, merged = self._pass(g, ne[g], store, True)
                if merged is None:
                    x[g] = s
                events.append((rounds, g, merged))
        return store, x[SEGS - 1], rounds, events

    def _pass(self, g, s, store, check):
        a = g * self.L
        for k in range(self.nk):
            if check and s == store[a + BATCH * k]:
                return s, k
            for q in range(BATCH):
                e = a + BATCH * k + q
                store[e] = s
                s = self.step(s, e)
        return s, None


def chains(data, **kw):
    """The block's three chains and its sequences' extra-bit counts in encoding order."""
    seq, ofb = parse(data)
    assert seq, "no sequences"
    llc = [ll_code(s[0]) for s in seq]
    mlc = [ml_code(s[1] - 3) for s in seq]
    ofc = [o.bit_length() - 1 for o in ofb]
    extra = [LL_BITS[a] + ML_BITS[b] + c for a, b, c in zip(llc, mlc, ofc)][::-1]
    return [Chain("ll", llc, **kw), Chain("of", ofc, **kw), Chain("ml", mlc, **kw)], extra


def trace(data, **kw):
    """-> {"nbSeq", "L", "modes", "chunk_bits" (the widest 64-step K4 append of the block: state bits
    plus LL, ML and OF extra bits), table name: {"mode", "log", "nbSeq", "L", "rounds", "reruns",
    "tags"}}.  Asserts the model's own consistency: stored states == the serial chain."""
    cs, extra = chains(data, **kw)
    n, L = cs[0].n, cs[0].L
    out = {"nbSeq": n, "L": L, "modes": tuple(c.mode for c in cs)}
    per_step = list(extra[:n])
    for c in cs:
        if c.mode == "rle":
            out[c.name] = dict(mode=c.mode, log=0, nbSeq=n, L=L, rounds=0, reruns=0, tags={"rle_chain"})
            continue
        ser, fin = c.serial()
        store, sfin, rounds, events = c.segmented()
        bad = next((e for e in range(SEGS * L) if store[e] != ser[e]), None)
        assert bad is None, f"{c.name}: the segmented scheme's state before step {bad} is {store[bad]}, the serial chain's {ser[bad]}"
        assert sfin == fin, f"{c.name}: final state {sfin}, serial {fin}"
        for e in range(1, n):
            per_step[e] += c.bits(ser[e], e)
        tags = {"short_warmup" if L < WARM else "full_warmup"}
        if rounds == 0 and n > 336:
            tags.add("no_fixup")
        if rounds == SEGS - 1 and (SEGS - 1) * L < n:
            tags.add("rounds_max")
            if L >= 64:
                tags.add("rounds_max_l64")
        seen = {}
        for r, g, merged in events:
            if merged is None:
                if c.nk >= 2 and g * L >= 1 and (g + 1) * L <= n:
                    tags.add("ran_to_end")
            else:
                assert merged > 0, "a re-run starts because its entry differs from the stored first state"
                tags.add("merge_last" if merged == c.nk - 1 else "merge_mid")
            if seen.setdefault(g, r) != r:
                tags.add("rerun_twice")
        if n % L and (n - 1) // L < SEGS - 1:
            tags.add("dead_tail")
        if c.clamped:
            tags.add("clamped")
        out[c.name] = dict(mode=c.mode, log=c.log, nbSeq=n, L=L, rounds=rounds, reruns=len(events), tags=tags)
    out["chunk_bits"] = max(sum(per_step[e0:e0 + 64]) for e0 in range(0, n, 64))
    return out


def frame_shape(frame):
    """(modes, nbSeq) of a one-block frame's compressed block, as zh_frames.walk reads them"""
    (b,) = F.walk(frame)
    assert b["type"] == "compressed", b["type"]
    return b["modes"], b["nseq"]

"""GPU parity of K1 at a block's edges (zh_lz.hip): the inserter waves run a window whose every
position lies below lim = n - ZH_HASH_READ through a body without the per-lane bounds test
(insert_window<.., EDGE = false>) and every other window -- the first one, which also honours a
dictionary's pmin, and the one or two that hold lim -- through the tested body; pass C of the
length phase folds the cap at ZH_MAX_MATCH into the cap at the block end.  Mode 0 is compared on
K1's raw records and literal bytes with the oracle's parse (test_gpu_k1._compare), levels 2 and 1
and the dictionary path on whole frames (test_gpu_k1_literals._frames).  Every comparison is exact.

Inputs are seeded random filler in which only the planted repeats match, blocks of at most four
windows (up to nine where miss-skip windows need them), with a 64-byte repeat in the first window so that the incompressibility probe lets the
block through; each batch is replicated to a few hundred blocks so that every workgroup meets
the edges, and the copies must agree with the first.  Before anything runs on the GPU the oracle
confirms on the CPU that each input reaches what it is for (orc_lz_match_info: the match at the
last searched position, no match at the first position past it, the capped lengths; the parse:
which windows take matches, which planted repeats a skipped window hides or a resumed one finds)."""
import ctypes

import numpy as np
import pytest

import test_gpu_k1 as K1
import zh_testlib as T
from test_gpu_k1 import _compare
from test_gpu_k1_literals import _frames
from zh_hash_model import P

pytestmark = pytest.mark.gpu

W = P["ZH_WINDOW"]
TILE = P["ZH_TILE"]
HR = P["ZH_HASH_READ"]
BATCH = 2 * TILE   # positions per inserter round trip
MAXM = 64          # ZH_MAX_MATCH
SRC = 300          # planted repeats copy from here (first window, inserted long before any edge)

assert W == 2048 and TILE == 128 and HR == 8


def _filler(seed, n):
    d = np.random.default_rng(seed).integers(0, 256, max(n, 0), dtype=np.uint8)
    if n >= 1200:
        d[1000:1064] = d[100:164]  # a match in the first window: the probe lets the block through
    return d


def _match_info(d):
    """The oracle's per-position best match (length, offset) with every tile searched."""
    O = T.oracle()
    d = np.ascontiguousarray(d, dtype=np.uint8)
    ln = np.zeros(len(d) + 1, dtype=np.uint8)
    of = np.zeros(len(d) + 1, dtype=np.uint16)
    O.orc_lz_match_info(d.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(len(d)), ln.ctypes.data_as(ctypes.c_void_p),
                        of.ctypes.data_as(ctypes.c_void_p))
    return ln, of


def _oracle_parse_pre(buf, pre):
    """The oracle's parse of buf[pre:] behind the history buf[:pre]: (ll, ml, off) and the last literals."""
    O = T.oracle()
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    seq = (ctypes.c_uint32 * (3 * (len(buf) // 5 + 2)))()
    last = ctypes.c_uint32(0)
    ns = O.orc_lz_parse_pre(buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(pre), ctypes.c_uint32(len(buf)), seq, ctypes.byref(last))
    return [(seq[3 * i], seq[3 * i + 1], seq[3 * i + 2]) for i in range(ns)], last.value


def _match_starts(d):
    """Start position and length of every match of the oracle's parse, and matches per window."""
    seqs, _ = K1.oracle_parse(d)
    out, p = [], 0
    for ll, ml, _ in seqs:
        p += ll
        out.append((p, ml))
        p += ml
    c = np.zeros(len(d) // W + 1, dtype=np.int64)
    for q, _ in out:
        c[q // W] += 1
    return out, c


def _tail_repeat(seed, n, s, chain=False, srcs=range(SRC, SRC + 60 * 11, 11)):
    """Filler of n bytes whose tail in[s, n) copies an earlier stretch of the first window, the
    byte before differing.  The stretch is one that both hash tables still hold when s is searched
    (a later position with the same hash would have taken its slot): the oracle finds it from s
    when the block is continued by eight more bytes, which makes every position up to n searched.
    chain: every searched position of the tail holds its own capped length too (none of the
    stretch's later positions lost its slots)."""
    for src in srcs:
        d = _filler(seed, n)
        if src + n - s + 3 > s:
            continue
        # the stretch is followed by zeros, like the block in K1's staging buffer: a length that
        # is not cut at the block end runs on into the padding
        d[src + n - s:src + n - s + 3] = 0
        d[s:n] = d[src:src + n - s]
        d[s - 1] = d[src - 1] ^ 0xFF
        ext = np.concatenate([d, np.full(HR, 0xFF, dtype=np.uint8)])
        ln, of = _match_info(ext)
        if ln[s] == min(MAXM, n - s) and of[s] == s - src and (not chain or all(ln[q] == min(MAXM, n - q) for q in range(s, n - HR))):
            return d, src
    raise AssertionError(f"no free source stretch for n={n} s={s}")


def _check_replicated(uniq, names, copies, levels=(2, 1)):
    """Mode 0: `copies` interleaved copies of the inputs in one K1 batch, every copy equal to the
    first; the inputs once more on their own against the oracle's parse; then the levels' frames."""
    uniq = [np.ascontiguousarray(d, dtype=np.uint8) for d in uniq]
    datas = uniq * copies
    assert len(datas) >= 256 and len(datas) * 65536 <= 24 << 20
    got = K1.k1_raw(datas)
    for i, (recs, lits, rle) in enumerate(got):
        r0, l0, f0 = got[i % len(uniq)]
        same = rle == f0 and np.array_equal(recs, r0) and (np.array_equal(lits, l0) if isinstance(l0, np.ndarray) else lits == l0)
        assert same, f"{names[i % len(uniq)]}: copy {i // len(uniq)} differs from the first"
    for (recs, lits, rle), (r0, l0, f0), nm in zip(K1.k1_raw(uniq), got, names):
        same = rle == f0 and np.array_equal(recs, r0) and (np.array_equal(lits, l0) if isinstance(l0, np.ndarray) else lits == l0)
        assert same, f"{nm}: the block on its own differs from its copies in the large batch"
    _compare(uniq, names)
    for level in levels:
        for f, d, nm in zip(_frames(level, uniq), uniq, names):
            assert f == T.oracle_frame(d, level=level), f"{nm}: level {level} frame differs from the oracle's"


# ---- 1. the inserter's edge / interior split ----------------------------------------------------

def _edge_sizes():
    lims = set()
    for base in (2 * W + 3 * BATCH, 3 * W + 5 * BATCH):          # a two-tile batch's first position
        lims |= {base - 1, base, base + 1}
    for base in (2 * W + 5 * TILE, 3 * W + 7 * TILE):            # a tile boundary that is no batch boundary
        lims |= {base - 1, base, base + 1}
    for base in (W, 2 * W, 3 * W, 4 * W):                        # a window boundary: the window below is
        lims |= {base - 1, base, base + 1}                       # interior from lim == base on
    lims |= {3 * W + 40, 3 * W + BATCH - 1}                      # inside the first batch of the last window
    ns = {lim + HR for lim in lims}
    ns |= {2 * W + x for x in (0, 1, HR - 1, HR, HR + 1, 255, 256, 257)}
    ns |= {1300, 2 * BATCH + 100}                                # lim inside the first window
    return sorted(ns)


def _edge_inputs():
    """Per size two blocks.  `below`: in[lim - 1, n) copies an earlier stretch and the byte before
    differs -- the last searched position carries a candidate and the block's last match.  `past`:
    in[lim, n) copies it and in[lim - 1] differs -- the oracle neither searches nor inserts lim, a
    wave that took the edge batch for an interior one finds an HR-byte match there."""
    datas, names = [], []
    for n in _edge_sizes():
        lim = n - HR
        for kind, s in (("below", lim - 1), ("past", lim)):
            d, _ = _tail_repeat(7000 + n, n, s)
            ln, _ = _match_info(d)
            if kind == "below":
                assert ln[lim - 1] == n - lim + 1, (n, ln[lim - 3:lim + 2].tolist())
                seqs, last = K1.oracle_parse(d)
                assert last == 0 and seqs[-1][1] == n - lim + 1, (n, seqs[-2:], last)
            else:
                assert not ln[lim - 2:].any(), n
                assert K1.oracle_parse(d)[1] >= HR + 2
            datas.append(d)
            names.append(f"{kind} n={n}")
    return datas, names


def test_inserter_edge_and_interior_windows():
    """(Whether the last positions below lim were inserted cannot be seen within one block: no
    later position of the block is searched, and the tables are cleared for the next block.  What
    shows is the search at lim - 1 and that lim itself is neither searched nor matched.)"""
    datas, names = _edge_inputs()
    _check_replicated(datas, names, -(-256 // len(datas)))


def test_blocks_below_one_batch_and_one_tile():
    """Sizes below one tile and one two-tile batch (the first window's body alone, lim inside its
    first batch), text so that the short blocks hold matches."""
    text = T.gen(T.DG_TEXT, 1, 0x5EED0041, 4096)
    sizes = (HR, HR + 1, 40, TILE - 1, TILE, TILE + HR, BATCH - 1, BATCH, BATCH + HR - 1, BATCH + HR, BATCH + HR + 1)
    datas = [np.tile(text[:max(n // 2, 1)], 3)[:n].copy() for n in sizes]
    names = [f"half-repeat n={n}" for n in sizes]
    assert any(len(K1.oracle_parse(d)[0]) for d in datas)
    _compare(datas, names)
    for level in (2, 1):
        for f, d, nm in zip(_frames(level, datas), datas, names):
            assert f == T.oracle_frame(d, level=level), f"{nm}: level {level}"


# ---- 2. pmin: blocks behind a dictionary prefix ------------------------------------------------

@pytest.mark.parametrize("pre", [2 * TILE, 3 * TILE - 1, 3 * TILE, 3 * TILE + 1, W - 1, W, W + 1])
def test_first_window_behind_dictionary_prefix(pre):
    """Level 3 behind a raw-content dictionary of `pre` bytes (the staged buffer is dictionary +
    block: pmin is the tile holding pre, the tables below it are precomputed).  Blocks that repeat
    the dictionary's tail across pre, its head, and a stretch of their own; sizes whose lim falls
    into the first window, onto the next window's start and three windows on."""
    rng = np.random.default_rng(900 + pre)
    dic = rng.integers(0, 256, pre, dtype=np.uint8)
    datas, names = [], []
    for n in (600, 2 * W - pre + HR, 2 * W - pre + HR + 1, 3 * W + 77):
        d = rng.integers(0, 256, n, dtype=np.uint8)
        d[:20] = dic[pre - 20:]            # continues the dictionary's last bytes ...
        d[20:40] = d[:20]                  # ... with period 20: the match at pre copies across pre
        d[100:160] = dic[10:70]            # the dictionary's head, below pmin (precomputed tables)
        d[300:340] = dic[pre - 100:pre - 60]
        d[500:560] = d[200:260]            # the block's own bytes, inserted by the first window
        datas.append(d)
        names.append(f"pre={pre} n={n}")
    dbytes = dic.tobytes()
    for d, nm in zip(datas, names):
        # the oracle's first match starts at pre (or pre + 1) and its source, 20 bytes back, crosses pre;
        # the dictionary's head is matched too
        seqs, _ = _oracle_parse_pre(np.concatenate([dic, d]), pre)
        assert seqs[0][0] <= 1 and seqs[0][1] >= 39 and seqs[0][2] == 20, (nm, seqs[:2])
        assert any(off == pre + 100 - 10 and ml >= 60 for _, ml, off in seqs), (nm, seqs[:6])
    want = [T.oracle_frame(d, dictionary=dbytes) for d in datas]
    copies = 64  # 256 blocks per call
    for f, w, nm in zip(_frames(3, datas * copies, dbytes), want * copies, names * copies):
        assert f == w, f"{nm}: frame differs from the oracle's"
    assert T.zstd_decompress(want[-1], len(datas[-1]), dictionary=dbytes) == datas[-1].tobytes()


# ---- 3. the length cap at the block end ---------------------------------------------------------

def _cap_inputs():
    """A repeat from position s to the block's last byte, s at lanes 0, 1, 62 and 63 of the last
    two length rounds and ten positions below the last round (a chain continuing into it from the
    round below): lengths min(64, n - s).  Sizes: the round below the last has its top position at
    n - 63, n - 64 and n - 65 (a 63-byte, a 64-byte and a capped 65-byte match at its lane 63), and
    the last round's lanes 62 / 63 are the last searched positions."""
    B = 9 * 64  # (a short block: few positions compete for the planted stretch's table slots)
    datas, names = [], []
    for n in (B + 126, B + 127, B + 128, B + 71, B + 72):
        lim = n - HR
        r0 = (lim - 1) // 64 * 64  # the last round with a searched position
        starts = {r + l for r in (r0 - 64, r0) for l in (0, 1, 62, 63)} | {r0 - 10, r0 - 64 - 10}
        for s in sorted(x for x in starts if x < lim):
            d, src = _tail_repeat(8000 + n, n, s, chain=True, srcs=range(150, 420, 7))
            ln, of = _match_info(d)
            assert ln[s] == min(MAXM, n - s) and of[s] == s - src, (n, s, int(ln[s]))
            # along the chain every searched position's length is capped by the block end or by 64
            for q in range(s, lim):
                assert ln[q] == min(MAXM, n - q), (n, s, q)
            datas.append(d)
            names.append(f"n={n} s={s} lane {s % 64} len {int(ln[s])}")
    lens = {int(nm.rsplit(" ", 1)[1]) for nm in names}
    assert {63, 64} <= lens and min(lens) <= HR + 2
    return datas, names


def test_match_lengths_capped_at_the_block_end():
    datas, names = _cap_inputs()
    _check_replicated(datas, names, -(-256 // len(datas)))


# ---- 4. miss-skip windows through both inserter bodies -----------------------------------------

def _skip_block(n, resume_last=False, seed=4100):
    """Random filler; window 0 holds the probe repeat, windows 1-3 nothing: windows 4 on are
    miss-skip windows (the parse took no match three windows before).  Window 4 holds a repeat
    past its first two tiles only: it does not resume (the inserters break after batch 0) and the
    repeat is never found.  Window 5 holds one inside its first two tiles: it resumes, and its
    second repeat, past them, is found.  Windows 6 and 7 skip again (3 and 4 took no match);
    window 8 searches whole (window 5 took matches): the block has left the mode."""
    d = _filler(seed + n, n)
    plants = {"w4_late": (4 * W + 1000, 400, 40), "w5_early": (5 * W + 100, 500, 40), "w5_late": (5 * W + 1200, 600, 40),
              "w8": (8 * W + 900, 700, 40)}
    if resume_last:
        k = (n - HR - 1) // W  # the last window: resumes from a repeat in its first tiles
        plants["last_early"] = (k * W + 30, 800, 30)
    for nm, (dst, src, ln) in plants.items():
        if dst + ln + 1 < n:
            d[dst:dst + ln] = d[src:src + ln]
            d[dst - 1] = d[src - 1] ^ 0xFF
            d[dst + ln] = d[src + ln] ^ 0xFF
    return d, plants


def _skip_inputs():
    datas, names = [], []
    # the block ends in window 4 (a skip window that is the last, lim in its first batch and past
    # it), in window 6 (after the resumed one), in window 7, and in window 8 (the mode left)
    for n, rl in ((4 * W + 100, False), (4 * W + 100, True), (4 * W + 700, False), (5 * W + 90, False), (5 * W + 1500, False),
                  (6 * W + 300, False), (6 * W + 300, True), (7 * W + 1000, False), (8 * W + 1100, False)):
        d, plants = _skip_block(n, rl)
        starts, c = _match_starts(d)
        found = {nm for nm, (dst, _, ln) in plants.items() if any(q <= dst + 8 and q + ml >= dst + ln - 8 and ml >= ln - 8 for q, ml in starts)}
        assert c[0] > 0 and not c[1:4].any(), (n, c.tolist())
        assert "w4_late" not in found, n                       # window 4 skipped and did not resume
        if n > 5 * W + 1300:
            assert {"w5_early", "w5_late"} <= found, (n, found)  # window 5 skipped and resumed
        if n > 6 * W:
            assert c[6] == 0 or rl
        if n > 8 * W + 1000:
            assert "w8" in found and c[7] == 0, (n, found)       # windows 6, 7 skipped; window 8 whole
        if rl:
            assert "last_early" in found, (n, found)
        datas.append(d)
        names.append(f"skip n={n}{' resume-last' if rl else ''}")
    return datas, names


def _probe_inputs():
    """Blocks whose first window takes no match: pure random (the probe ends the block for good)
    and random with repeats from the second window on (K1 ends the block at the probe, the repeat
    scan finds the repeats and the block is parsed again without the probe)."""
    rng = np.random.default_rng(4300)
    datas, names = [], []
    for n in (3 * W + 11, 6 * W):
        d = rng.integers(0, 256, n, dtype=np.uint8)
        datas.append(d.copy())
        names.append(f"random n={n}")
        for at in range(W + 300, n - 200, 700):
            d[at:at + 120] = d[at - 250:at - 130]
        starts, c = _match_starts(d)
        assert c[0] == 0 and c[1:].sum() >= 2, c.tolist()
        datas.append(d)
        names.append(f"random+repeats n={n}")
        assert K1.oracle_parse(datas[-2])[0] == []
    return datas, names


def test_miss_skip_windows_and_probe_redo():
    d1, n1 = _skip_inputs()
    d2, n2 = _probe_inputs()
    datas, names = d1 + d2, n1 + n2
    _check_replicated(datas, names, -(-256 // len(datas)))


# ---- 5. rounds per worker wave -------------------------------------------------------------------

def test_last_window_of_every_round_count():
    """Text (chains and queue entries in every round) cut so that the last window holds less than
    one round, less than one span (two or three rounds), and 1, 2 or 3 rounds for the waves whose
    spans the end falls into; full windows before it give every wave its whole span.  The single
    round per wave of a miss-skip window (NR = 1) is driven by test_miss_skip_windows_and_probe_redo."""
    text = T.gen(T.DG_TEXT, 1, 0x5EED0051, 65536)
    tails = (HR + 1, 20, 63, 64, 65, 64 + HR, 100, 128, 129, 191, 192, 200, 64 * 5 + 3, 64 * 7, 64 * 7 + HR + 1, 64 * 12 + 5,
             64 * 20 + 1, 64 * 27 + 9, 64 * 31 + 7, W - 1)
    datas = [text[:2 * W + t].copy() for t in tails]
    names = [f"text 2 windows + {t}" for t in tails]
    for d, t in zip(datas, tails):
        starts, c = _match_starts(d)
        assert c[0] > 10 and c[1] > 10
        if t >= 64:
            assert c[2] > 0, t  # the last window's rounds hold matches
    _check_replicated(datas, names, -(-256 // len(datas)))

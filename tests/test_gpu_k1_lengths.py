"""GPU parity of K1's length phase (zh_lz.hip span_lengths, xq_flush, ext8: per position the
candidates' common prefix, same-offset chains, the chain-end queue and its extension, the match
info and the take masks): K1's raw records and literal bytes equal the oracle's parse (the helpers
of test_gpu_k1.py) in mode 0; level 2 (mode 1, the same code with the short table only) through
the frame path against the oracle's frames.  Each input is seeded random filler -- only the planted
repeats match -- cut to the smallest block that reaches the code: chains starting at every lane
across round, span and window boundaries, a queue that fills more than once per span, equal and
different long / short candidates, exact match lengths around the 5- and 8-byte minimums and the
64-byte cap, matches that end at the block's last byte, and a window whose tables stay empty up to
its last tile.  Every comparison is exact."""
import numpy as np
import pytest

import zh_testlib as T
from zh_hash_model import P, hash_long, hash_short
from test_gpu_k1 import _compare, k1_raw, oracle_parse  # noqa: F401  (k1_raw, oracle_parse: _compare's parts)

pytestmark = pytest.mark.gpu

BLOCK = 65536
W = 2048    # K1's window
TILE = 128  # hash insertion granularity


assert P["ZH_WINDOW"] == W and P["ZH_TILE"] == TILE


def _filler(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _plant(d, dst, src, ln, exact=True):
    """d[dst:dst+ln] = d[src:src+ln]; with `exact` the bytes before and after differ, so the match
    at dst is ln bytes and the catch-up adds none."""
    d[dst:dst + ln] = d[src:src + ln]
    if exact:
        if dst + ln < len(d):
            d[dst + ln] = d[src + ln] ^ 0xFF
        d[dst - 1] = d[src - 1] ^ 0xFF


def _check(datas, names):
    datas = [np.ascontiguousarray(d, dtype=np.uint8) for d in datas]
    _compare(datas, names)
    import torch

    import cuda_zstd

    outs = cuda_zstd.Manager(2).compress_batch([torch.from_numpy(d).cuda() for d in datas])
    torch.cuda.synchronize()
    for o, d, nm in zip(outs, datas, names):
        assert o.cpu().numpy().tobytes() == T.oracle_frame(d, level=2), f"{nm}: level 2 frame differs from the oracle's"


def test_chain_start_at_every_lane_across_round_span_window():
    """A 300-byte repeat whose same-offset chain starts at lane j of round 30, j = 0..63: it crosses
    the round boundaries at 1984 (a span top: the window's last round belongs to another wave), 2048
    (the window's) and 2112, 2176 (inside the next window's first span)."""
    datas, names = [], []
    for j in range(64):
        d = _filler(1000 + j, 3 * W)
        _plant(d, 30 * 64 + j, 300, 300)
        datas.append(d)
        names.append(f"lane{j}")
    _check(datas, names)


def test_full_queue_runs_inside_text():
    """1 KiB runs of period 1, 2, 3, 5 and 7 inside text: a tile's positions of one phase all find the
    same earlier position, so every position is a chain end with 8 equal bytes -- 64 or 128 queue
    entries per round, the in-loop flush more than once per span."""
    d = T.gen(T.DG_TEXT, 1, 0x5EED0031, BLOCK).copy()
    rng = np.random.default_rng(41)
    at = 3000
    for period in (1, 2, 3, 5, 7):
        unit = rng.integers(0, 256, period, dtype=np.uint8)
        d[at:at + 1024] = np.tile(unit, 1024 // period + 1)[:1024]
        at += 1024 + 1500 + 37 * period  # (text between the runs; starts at varying lanes)
    short = d[:5 * W].copy()  # (the period 1 and 2 runs alone, in a block of 5 windows)
    _check([d, short], ["runs", "runs5w"])


def test_equal_and_different_candidates():
    """Block 0: a repeat whose nearest 5-byte and 8-byte occurrences are the same position (cS == cL;
    the short side takes the long side's extension at the chain's cut at the span top 1984).
    Block 1: next to such a repeat, one whose long-table slot was taken by a later position with the
    same long hash and other bytes -- the candidates differ and only the short one matches."""
    d0 = _filler(51, 3 * W)
    _plant(d0, 1950, 200, 120)
    d1 = _filler(52, 3 * W)
    _plant(d1, 1950, 200, 120)
    src, thief, dst = 500, 900, W + 700
    x = d1[src:src + 8]
    cand = np.random.default_rng(53).integers(0, 256, (1 << 20, 8), dtype=np.uint8)
    ok = (hash_long(cand) == hash_long(x)) & (hash_short(cand) != hash_short(x))
    assert ok.any()
    d1[thief:thief + 8] = cand[np.argmax(ok)]
    _plant(d1, dst, src, 40)
    # (the thief is the latest position of the long slot when dst's tile looks it up, and the
    # short slot still holds src)
    tl = {int(h): p for p, h in enumerate(hash_long(np.lib.stride_tricks.sliding_window_view(d1[:W + 640 + 7], 8)))}
    ts = {int(h): p for p, h in enumerate(hash_short(np.lib.stride_tricks.sliding_window_view(d1[:W + 640 + 7], 8)))}
    assert tl[int(hash_long(x))] == thief and ts[int(hash_short(x))] == src
    _check([d0, d1], ["equal", "equal+thief"])


def test_exact_lengths():
    """Matches of exactly 5, 6, 7 (short only), 8, 9, 63, 64 and 65 bytes (the cap is 64).  In the
    9-byte one the position after the start is an 8-byte match whose successor ends the chain with
    7 equal bytes; one 8-byte match follows a 9th equal byte placed before it the same way."""
    d = _filler(61, 3 * W)
    _plant(d, 1500, 40, 12)  # (a match in the first window: the block passes the probe)
    lens = (5, 6, 7, 8, 9, 63, 64, 65)
    for k, ln in enumerate(lens):
        for rep, base in enumerate((W + 50, 2 * W + 40)):  # (each length at two lane offsets)
            src = 100 + 160 * k + 80 * rep
            _plant(d, base + 230 * k + 7 * rep, src, ln)
    # 8 bytes after one equal byte: dst - 1 continues into dst, whose chain ends at dst + 1 with 7
    d[W + 1990:W + 1999] = d[1400:1409]
    d[W + 1999] = d[1409] ^ 0xFF
    d[W + 1989] = d[1399] ^ 0xFF
    _check([d], ["exact"])


def test_matches_to_the_last_byte():
    """A 100-byte repeat that ends with the block, n = 0, 1, 2, 3 mod 4: below one window, 2049 (one
    byte in the second window) and inside the third window."""
    datas, names = [], []
    for n in (1020, 1021, 1022, 1023, 2049, 2 * W + 2, 2 * W + 3, 2 * W + 4):
        d = _filler(70 + n, n)
        if n > W + 100:
            _plant(d, 1500, 40, 12)
        d[n - 100:n] = d[100:200]
        d[n - 101] = d[99] ^ 0xFF
        datas.append(d)
        names.append(f"n{n}")
    assert sorted({len(d) % 4 for d in datas}) == [0, 1, 2, 3]
    _check(datas, names)


def test_first_window_candidates_only_in_last_tile():
    """Filler whose positions up to the last tile of window 0 all hash to different slots of either
    table: the window's lookups find nothing until the last tile, which holds a repeat."""
    rng = np.random.default_rng(81)
    n0 = W - TILE
    d = np.zeros(3 * W, dtype=np.uint8)
    d[:7] = rng.integers(0, 256, 7, dtype=np.uint8)
    used_l, used_s = set(), {int(hash_short(d[i:i + 8])) for i in range(3)}
    for i in range(n0):  # byte i + 7 completes position i's 8 bytes (long) and position i + 3's 5 (short)
        for _ in range(64):
            d[i + 7] = rng.integers(0, 256)
            hl = int(hash_long(d[i:i + 8]))
            hs = int(hash_short(d[i + 3:i + 11]))
            if hl not in used_l and hs not in used_s:
                break
        else:
            raise AssertionError("no free slot")
        used_l.add(hl)
        used_s.add(hs)
    d[n0 + 7:] = rng.integers(0, 256, len(d) - n0 - 7, dtype=np.uint8)
    _plant(d, W - TILE + 20, 300, 90)
    _plant(d, W + 900, 700, 30)
    win = np.lib.stride_tricks.sliding_window_view(d[:n0 + 7], 8)
    assert len(set(hash_long(win).tolist())) == n0
    _check([d], ["late_tile"])

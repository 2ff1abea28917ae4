"""GPU parity of K1's window step where its waves hand buffers to each other (zh_lz.hip): wave 0
releases the previous window's match-info buffer to the inserters' dump as soon as it has gathered
every match's info -- before its scans and match-list entries -- and window k - 3's literal rounds
run in every kind of step (miss-skip windows, the drain steps after the last window, blocks of
fewer than four windows).  Mode 0 is compared on K1's raw records and literal bytes with the
oracle's parse (test_gpu_k1._compare); levels 2 and 1 on whole frames with the oracle's frames, as
tests/test_gpu_k1_literals.py does.  Every comparison is exact.

The early-release inputs make the gather and the entries pass long: a 2 KiB random head, then an
L-byte copy of an earlier stretch followed by one fresh random byte, repeated (L = 5, 6, 8, 12:
about 310 / 290 / 230 / 160 matches per window, so 5, 5, 4 and 3 passes of 64 matches).  Two
additions to that recipe, found with the oracle on the CPU: the head repeats 64 of its own bytes
(without a match in the block's first window the incompressibility probe ends the block and K1
parses nothing), and window 2 uses 20-byte copies (about 100 matches: a two-pass window between
five-pass ones).  Each batch holds 64 copies of the four inputs, interleaved: 256 blocks, one per
compute unit, so the inserters' dump races wave 0 in every workgroup at once; a race shows up as
copies that differ."""
import numpy as np
import pytest

import test_gpu_k1 as K1
import zh_testlib as T
from test_gpu_k1 import _compare, oracle_parse
from test_gpu_k1_literals import _frames

pytestmark = pytest.mark.gpu

BLOCK = 65536
W = 2048       # K1's window
COPIES = 64    # of each of the four dense inputs: 256 blocks, 16 MiB at the hook's 64 KiB stride
DENSE_L = (5, 6, 8, 12)


def _dense(L, n, sparse_window=2, sparse_L=20):
    rng = np.random.default_rng(100 + L)
    d = np.empty(n + 64, np.uint8)
    d[:W] = rng.integers(0, 256, W, dtype=np.uint8)
    d[1000:1064] = d[100:164]  # a match in the first window: the probe lets the block through
    pos = W
    while pos < n:
        ln = sparse_L if pos // W == sparse_window else L
        s = int(rng.integers(0, pos - ln))
        d[pos:pos + ln] = d[s:s + ln]
        d[pos + ln] = rng.integers(0, 256)
        pos += ln + 1
    return d[:n].copy()


def _matches_per_window(d):
    seqs, _ = oracle_parse(d)
    c = np.zeros((len(d) + W - 1) // W, dtype=np.int64)
    p = 0
    for ll, ml, _ in seqs:
        p += ll
        c[p // W] += 1
        p += ml
    return c


@pytest.mark.parametrize("size", [6144, 10000, 65536])
def test_early_release_under_load(size, monkeypatch):
    uniq = [_dense(L, size) for L in DENSE_L]
    names = [f"dense L={L} n={size}" for L in DENSE_L]
    c = _matches_per_window(uniq[0])
    print(f"matches per window, L={DENSE_L[0]} n={size}: {c.tolist()}")
    assert (c > 256).any(), "the densest input has no window of more than 256 matches"
    assert ((c >= 65) & (c <= 128)).any(), "the densest input has no window of 65-128 matches"
    datas = uniq * COPIES
    assert len(datas) >= 256 and len(datas) * BLOCK <= 16 << 20
    got = K1.k1_raw(datas)
    for i, (recs, lits, rle) in enumerate(got):
        r0, l0, f0 = got[i % len(uniq)]
        assert rle == f0 and np.array_equal(recs, r0) and lits == l0, f"{names[i % len(uniq)]}: copy {i // len(uniq)} differs from the first"
    # ... and the first copies, as this batch computed them, equal the oracle's parse
    monkeypatch.setattr(K1, "k1_raw", lambda ds: got[:len(ds)])
    _compare(uniq, names)
    monkeypatch.undo()
    for level in (2, 1):
        fr = _frames(level, datas)
        for i, f in enumerate(fr):
            assert f == fr[i % len(uniq)], f"{names[i % len(uniq)]}: level {level} copy {i // len(uniq)} differs from the first"
        for f, d, nm in zip(fr, uniq, names):
            assert f == T.oracle_frame(d, level=level), f"{nm}: level {level} frame differs from the oracle's"


def _lit_inputs():
    """Blocks of one to four windows, and text | 3 (and 6) windows of random | text, window-aligned
    and shifted by 5 bytes: the miss skip is entered and left with literals pending."""
    text = T.gen(T.DG_TEXT, 1, 0x5EED0031, BLOCK)
    rng = np.random.default_rng(41)
    datas, names = [], []
    for n in (100, 2047, 2048, 2049, 4096, 6144, 6145, 8193):
        datas.append(text[:n].copy())
        names.append(f"text{n}")
    for nr in (3, 6):
        for sh in (0, 5):
            a = 4 * W + sh
            datas.append(np.concatenate([text[:a], rng.integers(0, 256, nr * W, dtype=np.uint8), text[a:a + 8 * W + 77]]))
            names.append(f"text|rand{nr}w|text shift {sh}")
    return datas, names


def test_literal_rounds_short_blocks_and_miss_skip():
    datas, names = _lit_inputs()
    _compare(datas, names)
    for level in (2, 1):
        for f, d, nm in zip(_frames(level, datas), datas, names):
            assert f == T.oracle_frame(d, level=level), f"{nm}: level {level} frame differs from the oracle's"


@pytest.mark.parametrize("dict_size", [257, 1023])
def test_literal_rounds_behind_dictionary_prefix(dict_size):
    """The same blocks at level 3 behind a raw-content dictionary: `pre` sits inside the first
    window, so the first literal rounds start inside it."""
    datas, names = _lit_inputs()
    a = T.gen(T.DG_JSON, 1, 0x5EED0032, BLOCK)
    d = a[4096:4096 + dict_size].tobytes()
    for f, r, nm in zip(_frames(3, datas, d), datas, names):
        assert f == T.oracle_frame(r, dictionary=d), (dict_size, nm)
        assert T.zstd_decompress(f, len(r), dictionary=d) == r.tobytes(), (dict_size, nm)

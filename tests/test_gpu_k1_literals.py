"""GPU parity of K1's literal extraction (zh_lz.hip lit_rounds: a lane takes one aligned dword of
the window, its four literal bits and a v_perm_b32 compaction, 256 positions per round): K1's raw
records and literal bytes equal the oracle's parse (the helpers of test_gpu_k1.py) in mode 0; the
oracle's parse hook has no mode argument, so modes 1 and 2 (levels 2 and 1: the idle long-table
wave extracts whole windows, lanes = positions) are checked through the frame path against the
oracle's frames of that level.  The inputs put literal runs at every alignment against the extractor's dword, round
(256) and window (2,048) boundaries.  Every comparison is exact."""
import numpy as np
import pytest

import zh_testlib as T
from test_gpu_k1 import _compare, k1_raw, oracle_parse  # noqa: F401  (k1_raw, oracle_parse: _compare's parts)

pytestmark = pytest.mark.gpu

BLOCK = 65536
W = 2048   # K1's window
R = 256    # positions per literal round


def _frames(level, datas, dictionary=None):
    import torch

    import cuda_zstd

    m = cuda_zstd.Manager(level)
    if dictionary is not None:
        m.set_dictionary(cuda_zstd.Dictionary.load(dictionary))
    dev = [torch.from_numpy(np.ascontiguousarray(d)).cuda() for d in datas]
    outs = m.compress_batch(dev)
    torch.cuda.synchronize()
    return [o.cpu().numpy().tobytes() for o in outs]


def _check(datas, names):
    """Mode 0 on K1's raw output, modes 1 and 2 (levels 2, 1) on whole frames."""
    datas = [np.ascontiguousarray(d, dtype=np.uint8) for d in datas]
    _compare(datas, names)
    for level in (2, 1):
        for f, d, nm in zip(_frames(level, datas), datas, names):
            assert f == T.oracle_frame(d, level=level), f"{nm}: level {level} frame differs from the oracle's"


def test_literals_ragged_sizes():
    """Ragged last dwords, rounds and windows."""
    text = T.gen(T.DG_TEXT, 1, 0x5EED0021, BLOCK)
    sizes = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 6145, 65533, 65535, 65536)
    _check([text[:n].copy() for n in sizes], [f"text{n}" for n in sizes])


def test_literal_runs_across_dword_round_window_boundaries():
    """A 40-byte phrase repeated (one long match) with random bursts of 1-9 bytes at 256 k + d and
    2048 k + d, d in -5..5: literal runs that start and end at every offset modulo 4 and straddle
    the round and window boundaries."""
    rng = np.random.default_rng(31)
    phrase = np.frombuffer(b"the quick brown fox jumps over lazy dogs", np.uint8)
    assert len(phrase) == 40
    base = np.tile(phrase, BLOCK // 40 + 1)[:BLOCK]
    datas, names = [], []
    for L in (1, 2, 3, 4, 5, 6, 7, 8, 9, 0):  # 0: a random length per burst
        d = base.copy()
        for i, dd in enumerate(range(-5, 6)):
            for p in (R * (3 + 2 * i) + dd, W * (4 + 2 * i) + dd):
                n = L if L else int(rng.integers(1, 10))
                d[p:p + n] = rng.integers(0, 256, n, dtype=np.uint8)
        datas.append(d)
        names.append(f"bursts{L}")
    _check(datas, names)


def test_literal_window_transitions():
    """Whole windows without a literal (a period-7 repeat) next to windows that are all literals
    (2 KiB random stretches inside text), at window-aligned and unaligned offsets; a block whose
    last window is all literals and one whose first is."""
    rng = np.random.default_rng(32)
    text = T.gen(T.DG_TEXT, 1, 0x5EED0022, BLOCK)
    p7 = np.tile(np.arange(7, dtype=np.uint8) + 65, BLOCK // 7 + 1)

    def rnd(n):
        return rng.integers(0, 256, n, dtype=np.uint8)

    datas, names = [], []

    def add(nm, parts):
        names.append(nm)
        datas.append(np.concatenate(parts)[:BLOCK].copy())

    add("p7|rand|text|rand|p7", [p7[:2 * W], rnd(W), text[:2 * W], rnd(W), p7[:3 * W], text[2 * W:5 * W]])
    add("unaligned", [text[:3 * W + 5], rnd(W), p7[:2 * W + 3], rnd(W), text[3 * W:6 * W], p7[:W - 9], rnd(W)])
    add("text+p7 alternating", [x for k in range(8) for x in (text[k * W:(k + 1) * W], p7[:W])])
    add("last window literals", [text[:BLOCK - W], rnd(W)])
    add("last window literals ragged", [text[:30000], rnd(32768 + 100 - 30000)])
    add("first window literals", [rnd(W), text[:BLOCK - W]])
    add("first window literals, then p7", [rnd(W), p7[:4 * W], text[:4 * W]])
    _check(datas, names)


@pytest.mark.parametrize("dict_size", [257, 1021, 1022, 1023])
def test_literals_behind_dictionary_prefix(dict_size):
    """Level 3 with raw-content dictionaries whose staged tail is no multiple of 4 (nor of 2,048):
    the block starts at `pre` = the dictionary's size inside its first window and dword.  GPU
    frames equal the oracle's and decode with libzstd and the dictionary."""
    a = T.gen(T.DG_JSON, 2, 0x5EED0023, 40960)
    d = a[40960:40960 + dict_size].tobytes()
    text = T.gen(T.DG_TEXT, 1, 0x5EED0024, 40960)
    recs = [a[:4096].copy(), text[:4096].copy(), a[:40960].copy(), text]
    for f, r in zip(_frames(3, recs, d), recs):
        assert f == T.oracle_frame(r, dictionary=d), (dict_size, len(r))
        assert T.zstd_decompress(f, len(r), dictionary=d) == r.tobytes(), (dict_size, len(r))

"""Inputs of the long-distance matching tests, shared by the CPU model tests (test_ldm_model.py)
and the GPU tests (test_gpu_ldm.py).  Each builder returns (data, window_log, hash_log)."""
import functools

import numpy as np

import zh_testlib as T

CELL = 32768
KIB = 1024


def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def place(data, dst, src, ln):
    """Copy data[src:src+ln] to dst and make the bytes on both sides differ, so the run is exactly ln."""
    data[dst:dst + ln] = data[src:src + ln]
    if dst > 0 and src > 0:
        data[dst - 1] = data[src - 1] ^ 0x55
    if dst + ln < len(data):
        data[dst + ln] = data[src + ln] ^ 0x55


@functools.lru_cache(maxsize=None)
def case1():
    """random A (96 KiB) + random B (40,001 B) + A."""
    a, b = _rand(96 * KIB, 11), _rand(40001, 12)
    return np.concatenate([a, b, a]), 20, 20


GAPS = [("lead", 1), ("lead", 15), ("lead", 16), ("lead", 17), ("trail", 1), ("trail", 15), ("trail", 16), ("trail", 17)]


@functools.lru_cache(maxsize=None)
def case2(side, gap):
    """Text with an 8 KiB piece inserted again 200 KiB later, strictly inside cell 8: its first byte
    `gap` bytes after the cell's start (lead) or its last byte `gap` bytes before the cell's end (trail)."""
    text = T.gen(T.DG_TEXT, 6, 0x1D30 + gap, 65536)
    c0 = 8 * CELL
    q = c0 + gap if side == "lead" else c0 + CELL - gap - 8 * KIB
    p = q - 200 * KIB
    data = np.concatenate([text[:q], text[p:p + 8 * KIB], text[q:q + 40 * KIB]])
    data[q - 1] = data[p - 1] ^ 0x55
    data[q + 8 * KIB] = data[p + 8 * KIB] ^ 0x55
    return data, 20, 20


@functools.lru_cache(maxsize=None)
def case3():
    """The frame ends inside a duplicate: its last block is a one-sequence block."""
    x = _rand(100 * KIB, 31)
    filler = T.gen(T.DG_TEXT, 1, 0x33, 50000)
    return np.concatenate([x, filler, x[:70000]]), 20, 20


@functools.lru_cache(maxsize=None)
def case4(kind):
    if kind == "plain":  # a corpus frame: nothing repeats 64 bytes long further than 32 KiB back
        return T.gen(T.DG_JSON, 3, 0x44, 65536)[:190001].copy(), 20, 20
    if kind == "near":  # every repeat is 20,000 bytes back
        return np.concatenate([np.tile(_rand(20000, 40 + i), 2) for i in range(6)]), 20, 20
    if kind == "beyond":  # a repeat at distance 2^window_log + 1
        x = _rand(65537, 45)
        return np.concatenate([x, x[:30000]]), 16, 20
    assert kind == "edge"  # a repeat at distance exactly 2^window_log: used
    x = _rand(65536, 46)
    return np.concatenate([x, x[:30000]]), 16, 20


@functools.lru_cache(maxsize=None)
def case5(kind):
    """Offset selection inside cell 5 of a random frame; returns also the expected record."""
    data = _rand(7 * CELL, 50)
    c0 = 5 * CELL
    if kind == "longer":  # runs of 3 KiB and 5 KiB at two distances: the longer wins
        place(data, c0 + 100, 1000, 3 * KIB)
        place(data, c0 + 5000, 40000, 5 * KIB)
        want = (c0 + 5000, 5 * KIB, c0 + 5000 - 40000)
    elif kind == "six":  # six distances, the two longest runs last: only the first four are looked at
        lens = [2048, 2100, 2200, 2300, 3000, 4000]
        at = c0 + 50
        for k, ln in enumerate(lens):
            place(data, at, 3000 + 9000 * k, ln)
            if k == 3:
                want = (at, ln, at - (3000 + 9000 * k))
            at += ln + 300
    else:  # equal runs: the distance that appears first wins
        assert kind == "equal"
        place(data, c0 + 200, 2000, 3000)
        place(data, c0 + 8000, 50000, 3000)
        want = (c0 + 200, 3000, c0 + 200 - 2000)
    return data, 20, 20, want


@functools.lru_cache(maxsize=None)
def case6():
    """1 MiB of 16 KiB pieces drawn with repeats from 24 distinct ones, a 2^10-slot table: heavy eviction."""
    rng = np.random.default_rng(60)
    pool = [T.gen(T.DG_MIX, 1, 0x600 + i, 16 * KIB) for i in range(24)]
    return np.concatenate([pool[int(k)] for k in rng.integers(0, 24, 64)]), 22, 10


@functools.lru_cache(maxsize=None)
def case7(kind):
    if kind == "zeros":
        return np.zeros(256 * KIB, np.uint8), 20, 20
    if kind == "sampled-byte":  # a constant byte whose hash is a sample: every position is one, the per-cell cap decides
        import zh_ldm_model as M

        v = next(v for v in range(256) if M.is_sample(M.hashes(np.full(64, v, np.uint8)))[0])
        return np.full(256 * KIB, v, np.uint8), 20, 20
    return np.tile(np.array([3, 1, 4, 1, 5, 9, 2], np.uint8), 256 * KIB // 7 + 1)[:256 * KIB].copy(), 20, 20


@functools.lru_cache(maxsize=None)
def case10():
    """16 MiB, the second half equal to the first: distance 2^23, offset code 23."""
    half = T.gen(T.DG_MIX, 128, 0xA10, 65536)
    return np.concatenate([half, half]), 25, 20


def case10_records():
    """Case 10's records in closed form (test_ldm_model runs the model against it once)."""
    data, _, _ = case10()
    half = len(data) // 2
    cells = np.arange(len(data) // CELL, dtype=np.uint32)
    rec = np.stack([cells * CELL, np.full_like(cells, CELL), np.full_like(cells, half)], axis=1)
    rec[: half // CELL] = 0
    return rec


SMALL = {
    "case1": case1, "case3": case3, "case6": case6,
    **{f"case2-{s}{g}": functools.partial(case2, s, g) for s, g in GAPS},
    **{f"case4-{k}": functools.partial(case4, k) for k in ("plain", "near", "beyond", "edge")},
    **{f"case5-{k}": (lambda k=k: case5(k)[:3]) for k in ("longer", "six", "equal")},
    **{f"case7-{k}": functools.partial(case7, k) for k in ("zeros", "period7", "sampled-byte")},
}

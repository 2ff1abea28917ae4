"""The host model of a dictionary's precomputed tables (zh_dict_tables_model.py, the reference of
test_gpu_dictset.py::test_tables_equal_host_model) against a plain loop over the positions, with
the hashes in Python integers.  No GPU."""
import numpy as np
import pytest

import zh_dict_tables_model as M
from zh_hash_model import P


def loop_hashes(b):
    """(long slot, short slot) of the 8 bytes b."""
    b = [int(x) for x in b]
    lo = (b[0] | b[1] << 8 | b[2] << 16) * P["ZH_HK_L0"] + (b[3] | b[4] << 8 | b[5] << 16) * P["ZH_HK_L1"] + (b[6] | b[7] << 8) * P["ZH_HK_L2"]
    sh = (b[0] | b[1] << 8 | b[2] << 16) * P["ZH_HK_S0"] + (b[3] | b[4] << 8) * P["ZH_HK_S1"]
    return (lo & 0xFFFFFFFF) >> (32 - P["ZH_HASH_LOG_LONG"]), (sh & 0xFFFFFFFF) >> (32 - P["ZH_HASH_LOG_SHORT"])


def loop_k1(content):
    p = min(len(content), 65535)
    if p < 512:
        return 0, None
    tail = content[len(content) - p:]
    tl, ts = [0] * M.HL_SIZE, [0] * M.HS_SIZE
    for j in range(p - 256):  # in order: the latest position stays
        hl, hs = loop_hashes(tail[j:j + 8])
        tl[hl] = ts[hs] = j + 1
    return p, np.array(tl + ts, np.uint16)


def loop_deep(content):
    dp = min(len(content), 65536)
    split = (dp - 8) & ~3 if dp > 8 else 0
    if split < 64:
        return 0, 0, None, None
    tail = content[len(content) - dp:]
    head, prev = [0] * M.HS_SIZE, []
    for p in range(split):
        hs = loop_hashes(tail[p:p + 8])[1]
        prev.append(head[hs])
        head[hs] = p + 1
    return dp, split, np.array(prev, np.uint32), np.array(head, np.uint32)


def contents():
    rng = np.random.default_rng(0x5EED0E00)
    return {"random600": rng.integers(0, 256, 600, dtype=np.uint8), "random2000": rng.integers(0, 256, 2000, dtype=np.uint8),
            "constant": np.full(1500, 0x41, np.uint8), "period3": np.resize(np.array([1, 2, 3], np.uint8), 1501)}


@pytest.mark.parametrize("name", sorted(contents()))
def test_model_equals_loop(name):
    c = contents()[name]
    p, tabs = M.k1_tables(c)
    lp, ltabs = loop_k1(c)
    assert p == lp == len(c) and np.array_equal(tabs, ltabs)
    dp, split, prev, head = M.deep_chains(c)
    ldp, lsplit, lprev, lhead = loop_deep(c)
    assert (dp, split) == (ldp, lsplit) == (len(c), (len(c) - 8) & ~3)
    assert np.array_equal(prev, lprev) and np.array_equal(head, lhead)
    nl, ns, nh = [int(np.count_nonzero(t)) for t in (tabs[:M.HL_SIZE], tabs[M.HL_SIZE:], head)]
    if name == "constant":  # every position collides in one slot
        assert (nl, ns, nh) == (1, 1, 1) and tabs.max() == p - 256 and head.max() == split
        assert np.array_equal(prev, np.arange(split))
    elif name == "period3":
        assert (nl, ns, nh) == (3, 3, 3) and np.array_equal(prev[3:], np.arange(1, split - 2))
    else:
        assert ns > (p - 256) * 0.9 and nh > split * 0.9


def test_shapes():
    assert [M.k1_shape(n) for n in (1, 511, 512, 513, 65535, 65536, 131072)] == [0, 0, 512, 513, 65535, 65535, 65535]
    assert [M.deep_shape(n) for n in (1, 71, 72, 75, 76, 255, 65536, 65537)] == [(0, 0), (0, 0), (72, 64), (75, 64), (76, 68), (255, 244), (65536, 65528),
                                                                                  (65536, 65528)]
    assert M.k1_tables(np.zeros(511, np.uint8)) == (0, None) and M.deep_chains(np.zeros(71, np.uint8)) == (0, 0, None, None)

"""GPU parity of K2's table builders alone (csrc/zh_entropy.hip: fse_normalize_wave with its serial
fse_normalize_m2, fse_write_ncount_wave, fse_build_ctable_par, huf_build_ctable_par with
huf_set_max_height, huf_write_ctable_wave), run one wave per case through the library's
zh_test_fse_table / zh_test_huf_table hooks on K2's own LDS layout, against the oracle
(oracle/zstd_oracle.c orc_fse_normalize, orc_fse_write_ncount, orc_fse_build_ctable,
orc_huf_build_ctable, orc_huf_write_ctable).  Everything is an integer and compared exactly.

The cases are tests/zh_table_cases.py's: the directed ones (tests/test_table_cases.py shows on the
CPU that they meet every branch of the serial restatement, and pins the oracle to libzstd 1.4.9
on them), the grid and 1,000 seeded random ones per builder, all in one launch -- and once more in
reversed order, so that no result depends on what an earlier workgroup left in LDS.  Last, whole
inputs whose sequence tables take m2 in the real K2 path (tests/zh_table_inputs.py) are compressed
beside blocks that build no table; their frames equal the oracle's and decode."""
import numpy as np
import pytest

import test_gpu_chain as G
import zh_table_cases as C
import zh_table_inputs as I
import zh_testlib as T

pytestmark = pytest.mark.gpu

_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def fse_set():
    def make():
        cases = C.fse_directed() + C.fse_grid() + C.fse_random()
        return cases, [C.fse_oracle(c) for c in cases]
    return memo("fse", make)


def huf_set():
    def make():
        cases = C.huf_directed() + C.huf_grid() + C.huf_random()
        return cases, [C.huf_oracle(c) for c in cases]
    return memo("huf", make)


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import cuda_zstd

    return cuda_zstd


@pytest.mark.parametrize("order", ("forward", "reversed"))
def test_fse_tables_match_oracle(gpu, order):
    cases, want = fse_set()
    assert len(cases) >= 3000 and all(r.ret == c.tablelog and r.ncount for c, r in zip(cases, want))
    idx = list(range(len(cases)))[::-1 if order == "reversed" else 1]
    count = np.stack([cases[i].count for i in idx])
    par = np.array([[cases[i].maxsv, cases[i].total, cases[i].tablelog, cases[i].low] for i in idx], np.uint32)
    norm_lane, norm_st, nc, nc_size, st, sym = gpu._test_fse_table(count, par)
    bad = []
    for k, i in enumerate(idx):
        c, r = cases[i], want[i]
        n, t = c.maxsv + 1, 1 << c.tablelog
        what = None
        if norm_lane[k, :n].tolist() != r.norm.tolist() or norm_lane[k, n:].any():
            what = f"norm per lane {norm_lane[k, :n].tolist()} != {r.norm.tolist()}"
        elif norm_st[k, :n].tolist() != r.norm.tolist():
            what = f"norm[] as stored {norm_st[k, :n].tolist()} != {r.norm.tolist()}"
        elif int(nc_size[k]) != len(r.ncount) or nc[k, :len(r.ncount)].tobytes() != r.ncount:
            what = f"NCount {nc[k, :int(nc_size[k])].tobytes().hex()} != {r.ncount.hex()}"
        elif not (st[k, :t] == r.st).all():
            u = int(np.nonzero(st[k, :t] != r.st)[0][0])
            what = f"state {u}: {int(st[k, u])} != {int(r.st[u])}"
        elif not (sym[k, :n] == r.sym).all():
            s = int(np.nonzero((sym[k, :n] != r.sym).any(1))[0][0])
            what = f"symbol transform {s}: {sym[k, s].tolist()} != {r.sym[s].tolist()}"
        if what:
            bad.append(f"{c.name} (maxSV {c.maxsv}, total {c.total}, tableLog {c.tablelog}, low {c.low}): {what}")
    assert not bad, f"{len(bad)} of {len(cases)} cases differ ({order}); first: " + "; ".join(bad[:3])


@pytest.mark.parametrize("order", ("forward", "reversed"))
def test_huf_tables_match_oracle(gpu, order):
    cases, want = huf_set()
    assert len(cases) >= 3000 and all(r.hufflog for r in want)
    idx = list(range(len(cases)))[::-1 if order == "reversed" else 1]
    count = np.stack([cases[i].count for i in idx])
    par = np.array([[cases[i].maxsv, cases[i].maxbits] for i in idx], np.uint32)
    huff_log, hnb, hval, hdr, hdr_size = gpu._test_huf_table(count, par)
    bad = []
    for k, i in enumerate(idx):
        c, r = cases[i], want[i]
        what = None
        if int(huff_log[k]) != r.hufflog:
            what = f"huffLog {int(huff_log[k])} != {r.hufflog}"
        elif not (hnb[k] == r.nbits).all():
            s = int(np.nonzero(hnb[k] != r.nbits)[0][0])
            what = f"nbBits[{s}] {int(hnb[k, s])} != {int(r.nbits[s])}"
        elif not (hval[k] == r.val).all():
            s = int(np.nonzero(hval[k] != r.val)[0][0])
            what = f"val[{s}] {int(hval[k, s])} != {int(r.val[s])}"
        elif int(hdr_size[k]) != len(r.header) or hdr[k, :len(r.header)].tobytes() != r.header:
            what = f"header {hdr[k, :min(int(hdr_size[k]), 256)].tobytes().hex()} != {r.header.hex()}"
        if what:
            bad.append(f"{c.name} (maxSV {c.maxsv}, maxNbBits {c.maxbits}): {what}")
    assert not bad, f"{len(bad)} of {len(cases)} cases differ ({order}); first: " + "; ".join(bad[:3])


@pytest.mark.parametrize("level", I.LEVELS)
def test_inputs_that_take_m2_match_oracle(gpu, level):
    """Every input of zh_table_inputs at one level through the stream-ordered batch path, each
    followed by a block that builds no table (empty, raw, RLE, no sequences): oracle bytes, and
    libzstd and the GPU decode them.  tests/test_table_cases.py::test_inputs_reach_m2 shows which
    of these frames took m2 in which table at this level."""
    import torch

    f = G.fillers()
    items = []
    for i, c in enumerate(I.cases()):
        items += [c, f[i % 4]]
    assert any(I.REACH[n].get(level) for n, _ in I.cases())
    status, frames = G.compress_async(torch, items, level=level)
    G.check(items, status, frames, level=level, what=f"level {level}")
    full = [(n, d, fr) for (n, d), fr in zip(items, frames) if len(d)]
    for n, d, fr in full:
        assert T.zstd_decompress(fr, len(d)) == d.tobytes(), f"level {level} {n}: libzstd decode"
    m = gpu.Manager(level)
    back, st = m.decompress_batch([torch.from_numpy(np.frombuffer(fr, np.uint8).copy()).cuda() for _, _, fr in full], [len(d) for _, d, _ in full],
                                  raise_on_error=False)
    assert st == [0] * len(full), [(n, s) for (n, _, _), s in zip(full, st) if s]
    for (n, d, _), o in zip(full, back):
        assert o.cpu().numpy().tobytes() == d.tobytes(), f"level {level} {n}: GPU decode"

"""One COVER dictionary per group of samples in one device call (csrc/zh_dict_train.hip):
Dictionary.train_groups, DictionarySet.train and cuda_zstd_train_dictionaries_device must give, for
every group, the bytes of the host trainer (zh::cover_train through Dictionary.train on host bytes)
run on that group's samples alone.  Equality only, no tolerance.  Every group that is not empty on
purpose must give 256 .. dict_size bytes on the host, so that two empty results never "agree".
Corpora are a few hundred KiB per case.  The formulation without a GPU:
tests/test_dict_train_set_plan.py."""
import ctypes

import numpy as np
import pytest

import zh_testlib as T

pytestmark = pytest.mark.gpu


def _cut(corpus, sizes):
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert offs[-1] <= len(corpus)
    return [corpus[offs[i]:offs[i + 1]] for i in range(len(sizes))]


def _json(seed, sizes):
    return _cut(T.gen(T.DG_JSON, 1, seed, max(int(np.sum(sizes)), 1)), sizes)


def _u(seed, lo, hi, n):
    return [int(v) for v in np.random.default_rng(seed).integers(lo, hi + 1, n)]


def _host(samples, dict_size, k=0, d=0):
    """The host trainer on one group alone -> its bytes, or None where the host entry gives no
    dictionary (under 256 bytes).  Zero-size samples hold no position and are left out, as in
    tests/test_gpu_dict_train.py."""
    import cuda_zstd

    raw = [s.tobytes() for s in samples if len(s)]
    if not raw:
        return None
    try:
        return cuda_zstd.Dictionary.train(raw, dict_size, k, d).content()
    except cuda_zstd.ZstdError:
        return None


def _check_reference(want, dict_size, empty=()):
    for g, w in enumerate(want):
        if g in empty:
            assert w is None, f"group {g} was meant to give nothing"
        else:
            assert w is not None and 256 <= len(w) <= dict_size, f"group {g}: the host result does not test anything"


def _dev(samples):
    import torch

    return [torch.from_numpy(s.copy()).cuda() if len(s) else torch.empty(0, dtype=torch.uint8, device="cuda") for s in samples]


def _py(groups, dict_size, k, d, stream=None):
    import cuda_zstd

    got = cuda_zstd.Dictionary.train_groups([_dev(g) for g in groups], dict_size, k, d, stream=stream)
    return [None if x is None else x.content() for x in got]


def _c(groups, dict_size, k, d, short_by=0):
    """cuda_zstd_train_dictionaries_device through ctypes -> (rc, contents or None, statuses)."""
    import cuda_zstd
    import torch

    L = cuda_zstd.lib()
    samples = [s for g in groups for s in g]
    flat = torch.from_numpy(np.concatenate(samples + [np.empty(0, np.uint8)])).cuda()
    n, ng = len(samples), len(groups)
    sizes = (ctypes.c_size_t * n)(*[len(s) for s in samples])
    counts = (ctypes.c_size_t * ng)(*[len(g) for g in groups])
    need = L.cuda_zstd_train_dictionaries_device_get_temp_size(sizes, n, counts, ng, dict_size, k)
    assert need > 0
    temp = torch.empty(need, dtype=torch.uint8, device="cuda")
    hs = (ctypes.c_void_p * ng)(*[1] * ng)
    st = (ctypes.c_int * ng)(*[-1] * ng)
    rc = L.cuda_zstd_train_dictionaries_device(flat.data_ptr(), sizes, n, counts, ng, dict_size, k, d, temp.data_ptr(), need - short_by,
                                               torch.cuda.current_stream().cuda_stream, hs, st)
    return rc, [cuda_zstd.Dictionary(h).content() if h else None for h in hs], list(st)


def _both(groups, dict_size, k, d, empty=()):
    """Both entries against the host trainer per group -> the reference."""
    want = [_host(g, dict_size, k, d) for g in groups]
    _check_reference(want, dict_size, empty)
    got = _py(groups, dict_size, k, d)
    bad = [g for g in range(len(groups)) if got[g] != want[g]]
    assert not bad, f"train_groups: groups {bad} differ from the host trainer"
    rc, c, st = _c(groups, dict_size, k, d)
    assert rc == 0
    bad = [g for g in range(len(groups)) if c[g] != want[g]]
    assert not bad, f"C entry: groups {bad} differ from the host trainer"
    assert st == [12 if g in empty else 0 for g in range(len(groups))]
    return want


def test_mixed_groups_one_wave():
    groups = [_json(1, [300] * 64), _json(4, _u(4, 100, 3000, 37)), _json(8, [20000]), _json(9, _u(9, 0, 40, 300)),
              _cut(np.full(100000, 0x41, np.uint8), [2000] * 50)]
    want = _both(groups, 4096, 1024, 8)
    assert len(want[4]) == 1024  # the constant group: one segment, then only zero scores


def test_identical_groups_give_identical_dictionaries():
    """A, A, A: a look-back that crosses a group's start changes the second and the third."""
    a = _json(21, _u(21, 200, 2000, 30))
    want = _both([a, a, a], 4096, 1024, 8)
    assert want[0] == want[1] == want[2]


@pytest.mark.parametrize("k", [64, 1024])
def test_look_back_stops_at_the_group_boundary(k):
    """tests/test_gpu_dict_train.py::test_look_back_edges across a boundary: a 16-byte marker in the
    last seg - 1 positions of group 0 and again at the head of group 1, seg - 2, seg - 1 and seg
    positions after it."""
    seg, n = k - 8 + 1, 8192
    marker = np.arange(0xA0, 0xB0, dtype=np.uint8)
    for dist in (seg - 2, seg - 1, seg):
        a = T.gen(T.DG_RANDOM, 1, 0x5EED0D21, n).copy()
        b = T.gen(T.DG_RANDOM, 1, 0x5EED0D22, n).copy()
        p0 = n - 20
        assert n - p0 <= seg - 1
        p1 = p0 + dist - n
        for arr, at in ((a, 100), (a, p0), (b, p1), (b, p1 + 3000)):
            arr[at:at + 16] = marker
        _both([[a], [b]], 4096, k, 8)


def test_independent_control_state():
    """One wave: a group of many epochs, one that fills its dictionary, one under k bytes and one
    without samples.  The last two report 12 and leave the others alone."""
    groups = [_json(3, [4096] * 40), _json(5, [65536] * 3), _json(13, [1000]), []]
    _both(groups, 65536, 1024, 8, empty=(2, 3))


def test_more_groups_than_slots():
    """70 groups: the slots of the first 64 are used again by the second wave."""
    groups = [_json(100 + (0 if g == 64 else g), [1024] * 20) for g in range(70)]
    want = _both(groups, 2048, 1024, 8)
    assert want[0] == want[64]
    assert len(set(want)) == 69  # (every other pair differs, 63 / 64 / 65 among them: a slot's earlier group leaves nothing behind)


def test_look_back_from_global_memory():
    a = _json(14, [6000] * 20)
    _both([a, a], 65536, 40000, 8)


def test_one_group_equals_single_entry():
    import cuda_zstd
    import torch

    rng = np.random.default_rng(0x5EED0D1C)  # tests/test_gpu_dict_train.py's 200_ragged_1_5000 row
    samples = _json(2, [int(v) for v in rng.integers(1, 5001, 200)])
    want = _both([samples], 16384, 1024, 8)[0]
    L = cuda_zstd.lib()
    flat = torch.from_numpy(np.concatenate(samples)).cuda()
    n = len(samples)
    sizes = (ctypes.c_size_t * n)(*[len(s) for s in samples])
    temp = torch.empty(L.cuda_zstd_train_dictionary_device_get_temp_size(flat.numel(), n, 16384, 1024), dtype=torch.uint8, device="cuda")
    h = ctypes.c_void_p()
    rc = L.cuda_zstd_train_dictionary_device(flat.data_ptr(), sizes, n, 16384, 1024, 8, temp.data_ptr(), temp.numel(), None, ctypes.byref(h))
    assert rc == 0 and cuda_zstd.Dictionary(h.value).content() == want


def test_zero_size_samples():
    z = np.empty(0, np.uint8)
    a, b = _json(51, [500] * 20), _json(52, [500] * 20)
    _both([[z] + a + [z], [z, z, z], [z] + b + [z]], 4096, 1024, 8, empty=(1,))


def test_stream_order():
    """The samples are still being written by a copy queued on the same side stream when the call is made."""
    import cuda_zstd
    import torch

    samples = _json(3, [4096] * 40)
    want = [_host(samples[:20], 65536, 1024, 8), _host(samples[20:], 65536, 1024, 8)]
    _check_reference(want, 65536)
    staging = torch.from_numpy(np.stack(samples)).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.zeros_like(staging)
        t.copy_(staging, non_blocking=True)
        got = cuda_zstd.Dictionary.train_groups([t[:20], t[20:]], 65536, 1024, 8, stream=s)
    assert [x.content() for x in got] == want


def test_errors():
    import cuda_zstd
    import torch

    L = cuda_zstd.lib()
    groups = [_json(1, [300] * 64), _json(61, [300] * 64)]
    dict_size, k, d = 4096, 1024, 8
    want = [_host(g, dict_size, k, d) for g in groups]
    _check_reference(want, dict_size)
    rc, c, st = _c(groups, dict_size, k, d, short_by=1)
    assert rc == 7 and c == [None, None]
    samples = [s for g in groups for s in g]
    flat = torch.from_numpy(np.concatenate(samples)).cuda()
    n = len(samples)
    sizes = (ctypes.c_size_t * n)(*[len(s) for s in samples])
    counts = (ctypes.c_size_t * 4097)(64, 64)
    temp = torch.empty(L.cuda_zstd_train_dictionaries_device_get_temp_size(sizes, n, counts, 2, dict_size, k), dtype=torch.uint8, device="cuda")

    def call(szs, num, cnt, ng, dsize, outs=True):
        hs = (ctypes.c_void_p * 4097)(*[1] * 4097)
        rc = L.cuda_zstd_train_dictionaries_device(flat.data_ptr(), szs, num, cnt, ng, dsize, k, d, temp.data_ptr(), temp.numel(), None,
                                                   hs if outs else None, None)
        return rc, list(hs[:2])

    def valid():
        rc, hs = call(sizes, n, counts, 2, dict_size)
        assert rc == 0 and [cuda_zstd.Dictionary(h).content() for h in hs] == want

    valid()
    bad_counts = (ctypes.c_size_t * 2)(64, 63)
    assert call(sizes, n, bad_counts, 2, dict_size) == (2, [None, None])  # the counts do not sum to num_samples
    valid()
    bad_counts = (ctypes.c_size_t * 2)(64, 65)
    assert call(sizes, n, bad_counts, 2, dict_size) == (2, [None, None])
    valid()
    assert call(sizes, n, counts, 0, dict_size)[0] == 2  # no groups
    valid()
    assert call(sizes, n, counts, 4097, dict_size)[0] == 2
    valid()
    assert call(None, n, counts, 2, dict_size) == (2, [None, None])
    valid()
    assert call(sizes, n, None, 2, dict_size) == (2, [None, None])
    valid()
    assert call(sizes, n, counts, 2, dict_size, outs=False)[0] == 2
    valid()
    assert call(sizes, n, counts, 2, 100) == (2, [None, None])
    valid()
    assert call(sizes, n, counts, 2, 128 * 1024 + 1) == (2, [None, None])
    valid()


def test_end_to_end_trained_set(libzstd):
    import cuda_zstd
    import torch

    groups = [_cut(T.gen(T.DG_JSON, 64, 0x5EED0D30 + g, 4096), [4096] * 64) for g in range(4)]
    want = [_host(g, 16384) for g in groups]
    _check_reference(want, 16384)
    assert len(set(want)) == 4
    dset = cuda_zstd.DictionarySet.train([torch.from_numpy(np.stack(g)).cuda() for g in groups], 16384)
    assert len(dset) == 4
    recs = [_cut(T.gen(T.DG_JSON, 8, 0x5EED0D40 + g, 4096), [4096] * 8) for g in range(4)]
    items = [(recs[i % 4][i // 4], i % 4) for i in range(32)]
    idx = [e for _, e in items]
    frames = cuda_zstd.compress_batch_dicts([torch.from_numpy(r.copy()).cuda() for r, _ in items], dset, idx, level=3)
    torch.cuda.synchronize()
    for (r, e), f in zip(items, frames):
        fb = f.cpu().numpy().tobytes()
        assert fb == T.oracle_frame(r, dictionary=want[e])
        assert T.zstd_decompress(fb, len(r), dictionary=want[e]) == r.tobytes()
    back = cuda_zstd.decompress_batch_dicts(frames, dset, idx)
    for (r, _), o in zip(items, back):
        assert o.cpu().numpy().tobytes() == r.tobytes()
    small = [torch.from_numpy(np.stack(g)).cuda() for g in groups]
    small[2] = small[2][:1, :500]  # under k bytes
    with pytest.raises(cuda_zstd.ZstdError) as e:
        cuda_zstd.DictionarySet.train(small, 16384)
    assert e.value.code == 12 and "group 2" in str(e.value)

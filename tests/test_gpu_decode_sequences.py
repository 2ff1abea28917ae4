"""GPU decoder (zh_decode.hip), sequence semantics by construction: the hand-assembled vectors
of tests/zh_seqframes.py (test_seqframes.py shows what they cover and that libzstd decodes them to
the same bytes) decoded on the MI355X, bit-exact against the plain model.  Every block is decoded
as its buffer's only block (zh_dec_seq_kernel, resolve_off_masks, execute_block<ExecLds>) and after
a raw block (the serial reader, resolve_off, execute_block<DecLds>); a batch of 2,304 buffers takes
the split pipeline (zh_dec_tables_kernel)."""
import numpy as np
import pytest

import zh_seqframes as S

pytestmark = pytest.mark.gpu

A256 = lambda n: (n + 255) // 256 * 256  # noqa: E731


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _mgr(d=None):
    import cuda_zstd

    m = cuda_zstd.Manager(3)
    if d is not None:
        m.set_dictionary(cuda_zstd.Dictionary.load(d))
    return m


def _entries(vs):
    """(vector, alignment of the input's first byte modulo 16): vectors marked align16 at all 16."""
    return [(v, a) for v in vs for a in (range(16) if v.align16 else (0,))]


def _arena(torch, entries):
    """The inputs in one device allocation, entry k at a 256-byte boundary plus its alignment."""
    offs, cur = [], 0
    for v, a in entries:
        offs.append(cur + a)
        cur = A256(cur + a + len(v.bytes)) + 256
    host = np.zeros(cur, np.uint8)
    for (v, a), o in zip(entries, offs):
        host[o:o + len(v.bytes)] = np.frombuffer(v.bytes, np.uint8)
    dev = torch.from_numpy(host).cuda()
    assert dev.data_ptr() % 256 == 0
    return dev, [dev[o:o + len(v.bytes)] for (v, a), o in zip(entries, offs)]


def _check(entries, outs, st):
    bad = []
    for k, ((v, a), o, s) in enumerate(zip(entries, outs, st)):
        if v.expect == "nonzero":  # a Dictionary_ID no dictionary answers
            ok = s != 0
        elif v.expect:
            ok = s == v.expect
        else:
            ok = s == 0 and o.cpu().numpy().tobytes() == v.want
        if not ok:
            bad.append((k, repr(v), a, s))
    assert not bad, (len(bad), bad[:12])


def _run(torch, mgr, vs, total=None):
    entries = _entries(vs)
    if total:
        entries = [entries[k % len(entries)] for k in range(total)]
    keep, frames = _arena(torch, entries)
    outs, st = mgr.decompress_batch(frames, [v.cap for v, _ in entries], raise_on_error=False)
    assert len(outs) == len(entries)
    _check(entries, outs, st)
    return len(entries)


def test_sequence_vectors(torch_cuda):
    n = _run(torch_cuda, _mgr(), S.vectors())
    assert 200 < n < 1024


def test_sequence_vectors_split_pipeline(torch_cuda):
    """The whole set repeated cyclically to 2,304 buffers: the tables-only pass defers the Q
    forms.  Per-buffer capacities, each vector's own size: 245 MiB of output in all (the set with
    its 16 placements of the bits-per-step vectors is 30 MiB; a uniform capacity would be 19 GiB)."""
    assert _run(torch_cuda, _mgr(), S.vectors(), 2304) == 2304


@pytest.mark.parametrize("total", [None, 2304])
def test_dictionary_sequence_vectors(torch_cuda, total):
    _run(torch_cuda, _mgr(S.dictionary()), S.dict_vectors(), total)


def test_placement(torch_cuda):
    """One vector (41 KiB, a match across three windows) with its output at each alignment modulo
    4 and its input at each modulo 16, both forms, through BatchedDecompressor's pointer arrays;
    the bytes around each output stay untouched."""
    import cuda_zstd

    torch = torch_cuda
    vs = [v for v in S.vectors() if v.name == "W8192_span3_before"]
    assert [v.form for v in vs] == ["Q", "S"]
    entries = [(v, a) for v in vs for a in range(16) for _ in range(4)]
    keep, frames = _arena(torch, entries)
    n = len(entries)
    slot = A256(max(v.cap for v in vs) + 4) + 256
    out = torch.full((n * slot,), 0xEE, dtype=torch.uint8, device="cuda")
    o_off = [k * slot + 128 + k % 4 for k in range(n)]
    i64 = lambda x: torch.tensor(x, dtype=torch.int64, device="cuda")  # noqa: E731
    in_ptrs, in_sizes = i64([f.data_ptr() for f in frames]), i64([f.numel() for f in frames])
    out_ptrs, caps = i64([out.data_ptr() + o for o in o_off]), i64([v.cap for v, _ in entries])
    assert sorted({(int(p) % 16, (out.data_ptr() + o) % 4) for p, o in zip(in_ptrs.tolist(), o_off)}) == [(a, b) for a in range(16) for b in range(4)]
    sizes = torch.zeros(n, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    bd = cuda_zstd.BatchedDecompressor()
    temp = torch.empty(bd.temp_size(n, max(v.cap for v in vs)), dtype=torch.uint8, device="cuda")
    bd.decompress_async(in_ptrs, in_sizes, caps, max(v.cap for v in vs), out_ptrs, sizes, status, temp)
    torch.cuda.synchronize()
    assert status.tolist() == [0] * n and sizes.tolist() == [len(v.want) for v, _ in entries]
    host = out.cpu().numpy()
    for k, ((v, a), o) in enumerate(zip(entries, o_off)):
        assert host[o:o + len(v.want)].tobytes() == v.want, (k, v, a, o % 4)
        assert (host[k * slot:o] == 0xEE).all() and (host[o + len(v.want):(k + 1) * slot] == 0xEE).all(), (k, v, a, o % 4)

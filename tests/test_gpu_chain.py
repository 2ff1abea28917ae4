"""GPU parity on the directed chain inputs (tests/zh_chain_inputs.py): the frames the gfx950
kernels produce for them equal the oracle's byte for byte.  tests/test_chain_model.py proves on
the CPU, with a model of zh_fse_chain_kernel over the oracle's level-3 parse, that these inputs
force the chain kernel through every state of its segment scheme (no repair, all 20 rounds,
re-runs that merge mid-segment, at the last batch or never, dead tails, short and full warm-ups)
and put the sequence count on both sides of every geometry edge of the chain and packing
kernels; byte equality here proves the kernels handled them.  No round count is asserted on the
GPU (the kernel reports none outside diagnostic builds).

Three arrangements: every case at every level in one batch; the level-3 cases interleaved with
blocks that need no chain, at every wave position of the four-blocks-per-workgroup kernels and
every batch size mod 4; and the stream-ordered device-array path with and without a checksum."""
import numpy as np
import pytest

import zh_chain_inputs as C
import zh_testlib as T

pytestmark = pytest.mark.gpu

CS = 65536  # chunk slot of the stream-ordered path


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


_cases, _frames = [], {}


def cases():
    if not _cases:
        _cases.extend(C.cases())
    return _cases


def oracle_frame(name, d, level=3, checksum=False):
    k = (name, level, checksum)
    if k not in _frames:
        _frames[k] = T.oracle_frame(d, level=level, checksum=checksum)
    return _frames[k]


def fillers():
    """Blocks beside which a chain wave runs and which need no chain themselves: an empty item (no
    block: n == 0), a raw block, an RLE block and a 40-byte block without sequences (the entropy
    kernel finishes these: ZH_FF_NEED == 0)."""
    return [("empty", np.zeros(0, np.uint8)), ("random_1000", np.random.default_rng(7).integers(0, 256, 1000, dtype=np.uint8)),
            ("zeros_4096", np.zeros(4096, np.uint8)), ("no_sequences_40", np.arange(40, dtype=np.uint8))]


def compress_async(torch, items, level=3, checksum=False):
    """[(name, data)] through BatchedCompressor.compress_async -> (statuses, frames)"""
    import cuda_zstd

    n = len(items)
    buf = np.zeros(n * CS, np.uint8)
    for i, (_, d) in enumerate(items):
        buf[i * CS:i * CS + len(d)] = d
    dev = torch.from_numpy(buf).cuda()
    bc = cuda_zstd.BatchedCompressor(level, CS, checksum=checksum)
    slot = (bc.max_out(CS) + 255) // 256 * 256
    out = torch.empty(n * slot, dtype=torch.uint8, device="cuda")
    ar = torch.arange(n, dtype=torch.int64, device="cuda")
    in_sizes = torch.tensor([len(d) for _, d in items], dtype=torch.int64, device="cuda")
    out_sizes = torch.zeros(n, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    temp = torch.empty(bc.temp_size(n, CS), dtype=torch.uint8, device="cuda")
    bc.compress_async(dev.data_ptr() + ar * CS, in_sizes, CS, out.data_ptr() + ar * slot, out_sizes, status, temp)
    torch.cuda.synchronize()
    sizes, host = out_sizes.cpu().tolist(), out.cpu().numpy()
    return status.cpu().tolist(), [host[i * slot:i * slot + sizes[i]].tobytes() for i in range(n)]


def check(items, status, frames, level=3, checksum=False, what=""):
    for i, ((name, d), st, got) in enumerate(zip(items, status, frames)):
        if len(d) == 0:  # no frame: status 2 (invalid), size 0
            assert (st, got) == (2, b""), (what, i, name)
            continue
        want = oracle_frame(name, d, level, checksum)
        assert st == 0, (what, i, name, st)
        assert got == want, f"{what} item {i} {name}: GPU frame ({len(got)} B) != oracle ({len(want)} B)"


@pytest.mark.parametrize("level", C.LEVELS)
def test_chain_inputs_match_oracle(torch_cuda, level):
    """Every case in one compress_batch per level: oracle bytes, and the GPU decodes them.  (The
    census is a level-3 statement; the other levels add byte parity on the same inputs.)"""
    import cuda_zstd

    items = cases()
    m = cuda_zstd.Manager(level)
    outs = m.compress_batch([torch_cuda.from_numpy(d.copy()).cuda() for _, d in items])
    check(items, [0] * len(items), [o.cpu().numpy().tobytes() for o in outs], level, what=f"level {level}")
    back, st = m.decompress_batch(outs, [len(d) for _, d in items], raise_on_error=False)
    assert st == [0] * len(items), [(n, s) for (n, _), s in zip(items, st) if s]
    for (n, d), o in zip(items, back):
        assert o.cpu().numpy().tobytes() == d.tobytes(), f"level {level} {n}: GPU decode"


@pytest.mark.parametrize("shift", range(4))
def test_workgroup_neighbours(torch_cuda, shift):
    """The chain and packing kernels run four blocks per workgroup, one per wave; a wave whose
    block needs no chain returns at once beside waves that run one.  Every case is followed by
    a filler, and `shift` fillers come first: over the four shifts every case sits at every wave
    position, and the batch has 4k + 2, 4k + 3, 4k and 4k + 1 items (a last workgroup with one,
    two and three waves past the end)."""
    f = fillers()
    items = [f[k % 4] for k in range(shift)]
    for i, c in enumerate(cases()):
        items += [c, f[i % 4]]
    assert len(items) % 4 == (2 * len(cases()) + shift) % 4 and items[shift] is cases()[0] and items[shift + 2] is cases()[1]
    status, frames = compress_async(torch_cuda, items)
    check(items, status, frames, what=f"shift {shift}")


@pytest.mark.parametrize("checksum", (False, True))
def test_stream_ordered_path(torch_cuda, checksum):
    """The case list through compress_async (device arrays, 64 KiB chunk slots), without and with
    a content checksum."""
    items = cases()
    status, frames = compress_async(torch_cuda, items, checksum=checksum)
    assert status == [0] * len(items)
    check(items, status, frames, checksum=checksum, what=f"checksum {checksum}")

"""Long-distance matching on the GPU (csrc/zh_ldm.hip): the finder's plan against the numpy model
(zh_ldm_model.py), and the frames through libzstd and through the GPU decoder.

Inputs: zh_ldm_inputs.py (the CPU tests decode the model's own frames of the same inputs)."""
import numpy as np
import pytest

import zh_ldm_inputs as I
import zh_ldm_model as M
import zh_testlib as T

pytestmark = pytest.mark.gpu
KIB = 1024


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _manager(level, window_log, hash_log, on, checksum=False):
    import cuda_zstd

    m = cuda_zstd.Manager(level, checksum=checksum)
    assert cuda_zstd.lib().cuda_zstd_set_long_distance(m._h, int(on), window_log, hash_log) == 0
    return m


def _frame(torch, data, level, window_log, hash_log, on, checksum=False, stream=None):
    dev = torch.from_numpy(data).cuda()
    torch.cuda.synchronize()
    out = _manager(level, window_log, hash_log, on, checksum).compress(dev, stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes()


def _check(torch, data, window_log, hash_log, level=3, checksum=False):
    """The three things every case asserts; returns (plan, frame with matching on)."""
    import cuda_zstd

    want = M.plan(data, window_log, hash_log)
    got = cuda_zstd.ldm_plan(torch.from_numpy(data).cuda(), window_log, hash_log)
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, f"cells {bad[:8]}: finder {got[bad[:8]].tolist()} model {want[bad[:8]].tolist()}"
    on = _frame(torch, data, level, window_log, hash_log, True, checksum)
    assert T.zstd_decompress(on, len(data)) == data.tobytes(), "libzstd"
    back = cuda_zstd.decompress(torch.from_numpy(np.frombuffer(on, np.uint8).copy()).cuda(), len(data))
    assert back.cpu().numpy().tobytes() == data.tobytes(), "GPU decoder"
    return want, on


@pytest.mark.parametrize("level", [1, 3, 5])
def test_case1_repeated_block(torch_cuda, level):
    """A + B + A: the model hands all 96 KiB of the second A to 4 one-sequence blocks (it starts
    7,233 bytes into cell 4 and both its ends are found byte-exactly), so the ragged-end slack of
    2 x 1100 bytes and the 5 x 16 bytes of blocks bound the frame with room to spare."""
    data, wl, hl = I.case1()
    rec, on = _check(torch_cuda, data, wl, hl, level)
    saved, nblk = M.saved_bytes(M.partition(len(data), rec))
    assert (saved, nblk) == (96 * KIB, 4)
    off = _frame(torch_cuda, data, level, wl, hl, False)
    print(f"level {level}: on {len(on)} off {len(off)}")
    assert len(on) <= len(off) - 96 * KIB + 16 * 5 + 2 * 1100


@pytest.mark.parametrize("side,gap", I.GAPS)
def test_case2_three_block_cell(torch_cuda, side, gap):
    data, wl, hl = I.case2(side, gap)
    rec, on = _check(torch_cuda, data, wl, hl)
    c0 = 8 * I.CELL
    start = c0 + gap if side == "lead" else c0 + I.CELL - gap - 8 * KIB
    assert [tuple(r) for r in rec if r[1]] == [(start, 8 * KIB, 200 * KIB)]  # gap | one-sequence block | gap
    off = _frame(torch_cuda, data, 3, wl, hl, False)
    print(f"{side} {gap}: on {len(on)} off {len(off)}")
    assert len(on) < len(off)


@pytest.mark.parametrize("checksum", [False, True])
def test_case3_frame_ends_in_a_duplicate(torch_cuda, checksum):
    data, wl, hl = I.case3()
    rec, on = _check(torch_cuda, data, wl, hl, checksum=checksum)
    assert int(rec[-1][0]) + int(rec[-1][1]) == len(data)  # the last block is a one-sequence block
    tail = 4 if checksum else 0
    last = M.ldm_block(int(rec[-1][1]), int(rec[-1][2]), True)
    assert on[len(on) - tail - len(last):len(on) - tail] == last
    if checksum:
        assert on[4] & 4 and int.from_bytes(on[-4:], "little") == T.oracle().orc_xxh64(data.ctypes.data_as(T.vp), len(data)) & 0xFFFFFFFF


@pytest.mark.parametrize("kind", ["plain", "near", "beyond"])
def test_case4_nothing_to_find(torch_cuda, kind):
    data, wl, hl = I.case4(kind)
    rec, on = _check(torch_cuda, data, wl, hl)
    assert not rec[:, 1].any()
    assert on == _frame(torch_cuda, data, 3, wl, hl, False)
    assert on == T.oracle_frame(data, window_log=wl, level=3)


def test_case4_distance_equal_to_the_window(torch_cuda):
    data, wl, hl = I.case4("edge")
    rec, on = _check(torch_cuda, data, wl, hl)
    assert [tuple(r) for r in rec if r[1]] == [(65536, 30000, 1 << wl)]
    assert len(on) < len(_frame(torch_cuda, data, 3, wl, hl, False)) - 29000


@pytest.mark.parametrize("kind", ["longer", "six", "equal"])
def test_case5_offset_selection(torch_cuda, kind):
    data, wl, hl, want = I.case5(kind)
    rec, _ = _check(torch_cuda, data, wl, hl)
    assert [tuple(int(v) for v in r) for r in rec if r[1]] == [want]


def test_case6_small_table(torch_cuda):
    data, wl, hl = I.case6()
    assert M.table_log(len(data), hl) == 10
    rec, _ = _check(torch_cuda, data, wl, hl)
    assert rec[:, 1].any()


@pytest.mark.parametrize("kind", ["zeros", "period7", "sampled-byte"])
def test_case7_degenerate(torch_cuda, kind):
    data, wl, hl = I.case7(kind)
    _check(torch_cuda, data, wl, hl)


def test_case8_deterministic_across_streams(torch_cuda):
    data, wl, hl = I.case1()
    frames = [_frame(torch_cuda, data, 3, wl, hl, True, stream=torch_cuda.cuda.Stream()) for _ in range(2)]
    assert frames[0] == frames[1]


# cuda_zstd_get_compress_workspace_size(n) of a level-3 manager at the commit before this feature
PARENT_WORKSPACE = {1000: 233984, 65536: 597504, 65537: 895232, 236609: 2384384, 16 << 20: 152501504}


def test_case9_workspace(torch_cuda):
    import cuda_zstd

    data, wl, hl = I.case1()
    plain = cuda_zstd.Manager(3)
    for n, want in PARENT_WORKSPACE.items():
        assert plain.workspace_size(n) == want, n
    off, on = _manager(3, wl, hl, False), _manager(3, wl, hl, True)
    assert off.workspace_size(len(data)) == PARENT_WORKSPACE[len(data)]
    need = on.workspace_size(len(data))
    assert need > PARENT_WORKSPACE[len(data)]
    # exactly that much is enough
    lib = cuda_zstd.lib()
    import ctypes

    dev = torch_cuda.from_numpy(data).cuda()
    out = torch_cuda.empty(cuda_zstd.max_compressed_size(len(data)), dtype=torch_cuda.uint8, device="cuda")
    ws = torch_cuda.empty(need, dtype=torch_cuda.uint8, device="cuda")
    size = ctypes.c_size_t(out.numel())
    assert lib.cuda_zstd_compress(on._h, dev.data_ptr(), len(data), out.data_ptr(), ctypes.byref(size), ws.data_ptr(), need, 0) == 0
    assert T.zstd_decompress(out[:size.value].cpu().numpy().tobytes(), len(data)) == data.tobytes()
    size = ctypes.c_size_t(out.numel())
    assert lib.cuda_zstd_compress(on._h, dev.data_ptr(), len(data), out.data_ptr(), ctypes.byref(size), ws.data_ptr(), need - 512, 0) == 7


def test_case10_second_half_repeats_the_first(torch_cuda):
    """16 MiB: every cell of the second half is one block at distance 2^23.  The model's records
    for this input are I.case10_records(), which test_ldm_model.py::test_case10_model_and_bound
    checks by running the model (about 9 s, once, on the CPU side)."""
    import cuda_zstd

    data, wl, hl = I.case10()
    half = len(data) // 2
    dev = torch_cuda.from_numpy(data).cuda()
    got = cuda_zstd.ldm_plan(dev, wl, hl)
    assert (got == I.case10_records()).all()
    on = _frame(torch_cuda, data, 3, wl, hl, True)
    first = _frame(torch_cuda, data[:half].copy(), 3, wl, hl, False)
    print(f"on {len(on)} first half alone {len(first)}")
    assert T.zstd_decompress(on, len(data)) == data.tobytes()
    back = cuda_zstd.decompress(torch_cuda.from_numpy(np.frombuffer(on, np.uint8).copy()).cuda(), len(data))
    assert torch_cuda.equal(back, dev)
    assert len(on) <= len(first) + 16 * 256 + 2 * KIB


def test_entry_points_that_ignore_the_flag(torch_cuda, tmp_path):
    """tests/cpp_ldm/ldm_paths.cpp on case 1's input: compress() takes the flag; compress_batch of
    that one item (with the batch workspace size), a batch whose small item goes the cpu_threshold
    route, compress_with_history and compress() with a dictionary give the frames they give
    without it."""
    import os
    import subprocess

    exe = os.path.join(T.ROOT, "tests", "cpp_ldm", "ldm_paths")
    assert os.path.exists(exe), "build() makes tests/cpp_ldm/ldm_paths"
    data, _, _ = I.case1()
    path = tmp_path / "in.bin"
    data.tofile(path)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ldm paths OK" in r.stdout, r.stdout + r.stderr


def test_python_batch_and_zero(torch_cuda):
    """Manager(long_distance=...).compress_batch of one big chunk gives the frame of a manager
    without the flag; long_distance=0 is off."""
    import cuda_zstd

    data, wl, hl = I.case1()
    dev = torch_cuda.from_numpy(data).cuda()
    on, off = _manager(3, wl, hl, True), _manager(3, wl, hl, False)
    a, b = on.compress_batch([dev])[0], off.compress_batch([dev])[0]
    torch_cuda.cuda.synchronize()
    assert torch_cuda.equal(a, b)
    assert len(on.compress(dev)) < a.numel() - 90000
    zero, plain = cuda_zstd.Manager(3, long_distance=0), cuda_zstd.Manager(3)
    assert zero.workspace_size(len(data)) == plain.workspace_size(len(data))
    assert torch_cuda.equal(zero.compress(dev), plain.compress(dev))

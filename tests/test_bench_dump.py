"""bench.py --dump-outputs on CPU tensors: the files it writes, their types and size, the frame
checksum and sample against a numpy restatement, and that slot bytes past a frame's size (not
output) never reach the dump."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

NAMES = {"out_sizes", "status", "all_sizes", "frame_offsets", "frame_checksums", "frames_sample_index", "frames_sample"}


def fake_batch(n, slot, seed, tail_seed):
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(1, slot + 1, (n,), dtype=torch.int64, generator=g)
    sizes[0], sizes[1] = slot, 1  # a full slot and a one-byte frame
    frames = torch.randint(0, 256, (n, slot), dtype=torch.uint8, generator=g)
    # what lies past each frame differs with tail_seed
    junk = torch.randint(0, 256, (n, slot), dtype=torch.uint8, generator=torch.Generator().manual_seed(tail_seed))
    live = torch.arange(slot)[None, :] < sizes[:, None]
    d_out = torch.where(live, frames, junk).reshape(-1)
    return types.SimpleNamespace(n=n, slot=slot, dev=torch.device("cpu"), d_out=d_out, out_sizes=sizes,
                                 status=torch.zeros(n, dtype=torch.int32))


def dump(tmp, b, rank=0):
    offs = torch.cumsum(b.out_sizes, 0) - b.out_sizes
    bench.dump_outputs(str(tmp), b, b.out_sizes.clone(), offs, rank)
    return {f[:-4]: np.load(os.path.join(tmp, f)) for f in os.listdir(tmp)}


def test_dump_files_and_values(tmp_path):
    n, slot = 1500, 777  # more than one 1024-chunk checksum pass, more chunks than the sample
    b = fake_batch(n, slot, 1, 2)
    d = dump(tmp_path / "a", b)
    assert set(d) == NAMES
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert sum(a.nbytes for a in d.values()) <= 64 << 20
    raw = b.d_out.numpy().reshape(n, slot).astype(np.int64)
    sizes = b.out_sizes.numpy()
    w = np.arange(slot) % 251 + 1
    want = np.array([(raw[i, :sizes[i]] * w[:sizes[i]]).sum() for i in range(n)], np.float64)
    assert np.array_equal(d["frame_checksums"], want)
    assert np.array_equal(d["out_sizes"], sizes.astype(np.float64))
    assert np.array_equal(d["frame_offsets"], (np.cumsum(sizes) - sizes).astype(np.float64))
    idx = d["frames_sample_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE and len(set(idx)) == len(idx) and idx.min() >= 0 and idx.max() < n
    assert d["frames_sample"].shape == (len(idx), slot)
    for row, i in zip(d["frames_sample"], idx):
        assert np.array_equal(row[:sizes[i]], raw[i, :sizes[i]]) and not row[sizes[i]:].any()
    # same outputs, other bytes past the frames: the same dump
    d2 = dump(tmp_path / "b", fake_batch(n, slot, 1, 3))
    assert all(np.array_equal(d[k], d2[k]) for k in NAMES)


def test_dump_small_batch_and_rank_suffix(tmp_path):
    b = fake_batch(5, 300, 4, 5)
    d = dump(tmp_path, b, rank=2)
    assert set(d) == {k + "_rank2" for k in NAMES}
    assert np.array_equal(d["frames_sample_index_rank2"], np.arange(5, dtype=np.float64))

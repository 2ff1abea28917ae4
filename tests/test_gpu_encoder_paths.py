"""GPU parity on the directed encoder inputs (tests/zh_edge_inputs.py): the frames the gfx950
kernels produce for them equal the oracle's byte for byte at levels 1, 2, 3, 5 and 9, reach the
same entropy-stage paths the CPU census proves for the oracle (tests/test_encoder_paths.py:
sequence tables in RLE mode, RLE literals, raw literals with each header size, one- and
four-stream Huffman with direct and FSE-compressed weights, every size boundary), decode with
libzstd and decode on the GPU.  Variants: frames with a content checksum, and inputs at odd
byte offsets inside one buffer (the raw- and RLE-literal copies realign their source)."""
import numpy as np
import pytest

import test_encoder_paths as P
import zh_edge_inputs as E
import zh_frames as F
import zh_testlib as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def _check(level, names, datas, frames, oracle_frames):
    for n, d, got, want in zip(names, datas, frames, oracle_frames):
        assert got == want, f"level {level} {n}: GPU frame ({len(got)} B) != oracle ({len(want)} B)"
        assert T.zstd_decompress(got, len(d)) == d.tobytes(), f"level {level} {n}: libzstd round trip"
    got = F.features(frames)
    assert got >= P.required(level), sorted(P.required(level) - got)


def _gpu_decode(torch, level, names, datas, dev_frames):
    import cuda_zstd

    outs, st = cuda_zstd.Manager(level).decompress_batch(dev_frames, [len(d) for d in datas], raise_on_error=False)
    assert st == [0] * len(datas), [(n, s) for n, s in zip(names, st) if s]
    for n, d, o in zip(names, datas, outs):
        assert o.cpu().numpy().tobytes() == d.tobytes(), f"level {level} {n}: GPU decode"


@pytest.mark.parametrize("level", E.LEVELS)
def test_edge_inputs_match_oracle(torch_cuda, level):
    import cuda_zstd

    ref = P.oracle_frames(level)
    names = list(ref)
    datas = [ref[n][0] for n in names]
    outs = cuda_zstd.Manager(level).compress_batch([torch_cuda.from_numpy(d.copy()).cuda() for d in datas])
    _check(level, names, datas, [o.cpu().numpy().tobytes() for o in outs], [ref[n][1] for n in names])
    _gpu_decode(torch_cuda, level, names, datas, outs)


def test_edge_inputs_with_checksum(torch_cuda):
    """The stream-ordered device-array path with a content checksum (FHD flag + the low 32 bits
    of XXH64 after the last block), level 3."""
    import cuda_zstd

    torch, level, cs = torch_cuda, 3, 128 * 1024
    ref = P.oracle_frames(level)
    names = list(ref)
    datas = [ref[n][0] for n in names]
    n = len(datas)
    buf = np.zeros(n * cs, np.uint8)
    for i, d in enumerate(datas):
        buf[i * cs:i * cs + len(d)] = d
    dev = torch.from_numpy(buf).cuda()
    bc = cuda_zstd.BatchedCompressor(level, cs, checksum=True)
    slot = (bc.max_out(cs) + 255) // 256 * 256
    out = torch.empty(n * slot, dtype=torch.uint8, device="cuda")
    ar = torch.arange(n, dtype=torch.int64, device="cuda")
    in_sizes = torch.tensor([len(d) for d in datas], dtype=torch.int64, device="cuda")
    out_sizes = torch.zeros(n, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    temp = torch.empty(bc.temp_size(n, cs), dtype=torch.uint8, device="cuda")
    bc.compress_async(dev.data_ptr() + ar * cs, in_sizes, cs, out.data_ptr() + ar * slot, out_sizes, status, temp)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n
    sizes, host = out_sizes.cpu().tolist(), out.cpu().numpy()
    frames = [host[i * slot:i * slot + sizes[i]].tobytes() for i in range(n)]
    _check(level, names, datas, frames, [T.oracle_frame(d, level=level, checksum=True) for d in datas])
    assert "checksum" in F.features(frames)
    _gpu_decode(torch, level, names, datas, [out[i * slot:i * slot + sizes[i]] for i in range(n)])


@pytest.mark.parametrize("shift", range(4))
def test_edge_inputs_unaligned(torch_cuda, shift):
    """Inputs at odd offsets inside one buffer, level 3; over the four shifts every input starts
    at every byte alignment."""
    import cuda_zstd

    level = 3
    ref = P.oracle_frames(level)
    names = list(ref)
    datas = [ref[n][0] for n in names]
    offs, pos = [], shift
    for i, d in enumerate(datas):
        pos += i % 4 + 1  # 1..4 bytes of padding
        offs.append(pos)
        pos += len(d)
    buf = np.full(pos + 16, 0xEE, np.uint8)
    for o, d in zip(offs, datas):
        buf[o:o + len(d)] = d
    dev = torch_cuda.from_numpy(buf).cuda()
    outs = cuda_zstd.Manager(level).compress_batch([dev[o:o + len(d)] for o, d in zip(offs, datas)])
    _check(level, names, datas, [o.cpu().numpy().tobytes() for o in outs], [ref[n][1] for n in names])

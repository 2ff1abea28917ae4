"""The three plans of the compress pipeline write the same frames: Manager.compress_batch plans on
the host, BatchedCompressor.compress_async on the device (zh_plan_kernel), compress_levels_async on
the device with one level per item (zh_plan_levels_kernel); all three build their descriptors with
csrc/zh_block_plan.h.  One batch whose sizes sit on every branch of that rule (one block, the
32 KiB split of a dictionary frame, 64 KiB, history blocks with a short tail), every item padded to
the five block slots of the largest."""
import json
import os

import numpy as np
import pytest

import zh_testlib as T

pytestmark = pytest.mark.gpu

SIZES = [1, 32767, 32768, 32769, 65536, 65537, 98305, 163840]
MAX_CHUNK = max(SIZES)


def batch():
    kinds = [T.DG_TEXT, T.DG_JSON, T.DG_MIX, T.DG_SOURCE]
    return [T.gen(kinds[i % 4], 1, 0x5EED0C00 + i, n) for i, n in enumerate(SIZES)]


def device_route(datas, level, dictionary=None, levels=False):
    """compress_async (levels: compress_levels_async at `level` for every item) -> frames."""
    import torch

    import cuda_zstd

    n = len(datas)
    bc = cuda_zstd.BatchedCompressor(level, 65536)
    if dictionary is not None:
        bc.set_dictionary(dictionary)
    slot = (bc.max_out(MAX_CHUNK) + 255) // 256 * 256
    ins = [torch.from_numpy(d).cuda() for d in datas]
    out = torch.zeros(n * slot, dtype=torch.uint8, device="cuda")
    in_ptrs = torch.tensor([t.data_ptr() for t in ins], dtype=torch.int64, device="cuda")
    in_sizes = torch.tensor([len(d) for d in datas], dtype=torch.int64, device="cuda")
    out_ptrs = torch.tensor([out.data_ptr() + i * slot for i in range(n)], dtype=torch.int64, device="cuda")
    out_sizes = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    need = bc.temp_size_levels(n, MAX_CHUNK) if levels else bc.temp_size(n, MAX_CHUNK)
    temp = torch.empty(need, dtype=torch.uint8, device="cuda")
    if levels:
        bc.compress_levels_async(in_ptrs, in_sizes, torch.full((n,), level, dtype=torch.int32, device="cuda"), MAX_CHUNK, out_ptrs, out_sizes,
                                 status, temp)
    else:
        bc.compress_async(in_ptrs, in_sizes, MAX_CHUNK, out_ptrs, out_sizes, status, temp)
    torch.cuda.synchronize()
    bc.close()
    assert status.cpu().tolist() == [0] * n
    sizes, host = out_sizes.cpu().tolist(), out.cpu().numpy()
    return [host[i * slot:i * slot + sizes[i]].tobytes() for i in range(n)], need


def host_route(datas, level, dictionary=None):
    import torch

    import cuda_zstd

    m = cuda_zstd.Manager(level)
    if dictionary is not None:
        m.set_dictionary(dictionary)
    frames = [f.cpu().numpy().tobytes() for f in m.compress_batch([torch.from_numpy(d).cuda() for d in datas])]
    m.close()
    return frames


@pytest.mark.parametrize("level", [1, 3, 5])
def test_three_routes_one_frame_list(libzstd, level):
    datas = batch()
    host = host_route(datas, level)
    device, _ = device_route(datas, level)
    by_levels, _ = device_route(datas, level, levels=True)
    for i, d in enumerate(datas):
        assert device[i] == host[i], (i, "device plan")
        assert by_levels[i] == host[i], (i, "levels plan")
        assert T.zstd_decompress(host[i], len(d)) == d.tobytes(), i


@pytest.mark.parametrize("level", [3, 5])
def test_two_routes_with_a_dictionary(libzstd, level):
    """A raw-content 40 KiB dictionary: below ZH_DEEP_LEVEL a frame over 32 KiB is cut into 32 KiB
    blocks and the first sees 32 KiB of the content, at level 5 frames up to 64 KiB stay one block
    behind all of it.  The handle's workspace size is the recorded one."""
    import cuda_zstd

    datas = batch()
    content = T.gen(T.DG_JSON, 1, 0x5EED0C01, 20 * 1024).tobytes() + T.gen(T.DG_TEXT, 1, 0x5EED0C00, 20 * 1024).tobytes()
    d = cuda_zstd.Dictionary.load(content)
    host = host_route(datas, level, d)
    device, need = device_route(datas, level, d)
    with open(os.path.join(T.GOLDEN, "temp_sizes.json")) as f:
        assert need == json.load(f)["dict_batched_temp"][str(level)]
    plain = host_route(datas, level)
    for i, data in enumerate(datas):
        assert device[i] == host[i], i
        assert T.zstd_decompress(host[i], len(data), dictionary=content) == data.tobytes(), i
    assert host != plain  # the dictionary is used
    d.close()

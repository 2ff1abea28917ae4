"""COVER training on the device (csrc/zh_dict_train.hip): Dictionary.train on CUDA tensors,
cuda_zstd_train_dictionary_device and the C++ entries with device samples must give the bytes
of the host trainer (zh::cover_train through cuda_zstd_train_dictionary_params / Dictionary.train
on host bytes) for the same samples.  Equality only, no tolerance.  Corpora are at most a few
hundred KiB (one row: 2 MiB), where the host trainer takes milliseconds."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import zh_testlib as T

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(T.ROOT, "tests", "cpp_train", "dict_train")


def _cut(corpus, sizes):
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert offs[-1] <= len(corpus)
    return [corpus[offs[i]:offs[i + 1]] for i in range(len(sizes))]


def _json(seed, sizes):
    return _cut(T.gen(T.DG_JSON, 1, seed, max(int(np.sum(sizes)), 1)), sizes)


@functools.lru_cache(maxsize=None)
def _rows():
    rng = np.random.default_rng(0x5EED0D1C)
    u = lambda lo, hi, n: [int(v) for v in rng.integers(lo, hi + 1, n)]
    return {
        # name: (samples, dict_size, k, d)
        "64x300": (_json(1, [300] * 64), 4096, 1024, 8),
        "200_ragged_1_5000": (_json(2, u(1, 5000, 200)), 16384, 1024, 8),
        "40x4096_dict64k": (_json(3, [4096] * 40), 65536, 1024, 8),
        "37_k256_d6": (_json(4, u(100, 3000, 37)), 8192, 256, 6),
        "3x65536": (_json(5, [65536] * 3), 32768, 1024, 8),
        "50x2000_random": (_cut(T.gen(T.DG_RANDOM, 1, 6, 100000), [2000] * 50), 4096, 1024, 8),
        "50x2000_constant": (_cut(np.full(100000, 0x41, np.uint8), [2000] * 50), 4096, 1024, 8),
        "1x20000": (_json(8, [20000]), 4096, 1024, 8),
        "300_tiny_0_40": (_json(9, u(0, 40, 300)), 4096, 1024, 8),
        "512x4096_fixture": (_cut(T.gen(T.DG_JSON, 512, 0x5EED0005, 4096), [4096] * 512), 16384, 1024, 8),
        "30_dict128k": (_json(11, u(500, 9000, 30)), 131072, 1024, 8),
        "25x1100_k2048_d4": (_json(12, [1100] * 25), 2048, 2048, 4),
        "1x1024_N_eq_k": (_json(13, [1024]), 256, 1024, 8),
        # beyond the issue's table: the look-back from global memory (seg - 1 + tile > 64 KiB of LDS)
        "20x6000_k40000": (_json(14, [6000] * 20), 65536, 40000, 8),
    }


NAMES = ["64x300", "200_ragged_1_5000", "40x4096_dict64k", "37_k256_d6", "3x65536", "50x2000_random", "50x2000_constant", "1x20000",
         "300_tiny_0_40", "512x4096_fixture", "30_dict128k", "25x1100_k2048_d4", "1x1024_N_eq_k", "20x6000_k40000"]


def _host(samples, dict_size, k=0, d=0):
    import cuda_zstd

    # The host C entries refuse zero-size samples, zh::cover_train does not: an empty sample
    # holds no position, so it changes neither dm nor freq, and the host trainer's bytes for the
    # samples without them are its bytes with them (tests/cpp/dict_train_check.cpp runs that
    # shape through zh::cover_train itself).  The device calls get every sample.
    return cuda_zstd.Dictionary.train([s.tobytes() for s in samples if len(s)], dict_size, k, d).content()


def _dev_tensors(samples):
    import torch

    return [torch.from_numpy(s.copy()).cuda() if len(s) else torch.empty(0, dtype=torch.uint8, device="cuda") for s in samples]


def _c_device(samples, dict_size, k, d, short_by=0):
    """cuda_zstd_train_dictionary_device through ctypes -> (rc, content or None)."""
    import cuda_zstd
    import torch

    L = cuda_zstd.lib()
    flat = torch.from_numpy(np.concatenate(samples)).cuda()
    n = len(samples)
    sizes = (ctypes.c_size_t * n)(*[len(s) for s in samples])
    need = L.cuda_zstd_train_dictionary_device_get_temp_size(flat.numel(), n, dict_size, k)
    temp = torch.empty(need, dtype=torch.uint8, device="cuda")
    h = ctypes.c_void_p()
    rc = L.cuda_zstd_train_dictionary_device(flat.data_ptr(), sizes, n, dict_size, k, d, temp.data_ptr(), need - short_by,
                                             torch.cuda.current_stream().cuda_stream, ctypes.byref(h))
    if not h.value:
        return rc, None
    return rc, cuda_zstd.Dictionary(h.value).content()


@pytest.mark.parametrize("name", NAMES)
def test_shape_table_device_equals_host(name):
    import cuda_zstd

    assert sorted(NAMES) == sorted(_rows())
    samples, dict_size, k, d = _rows()[name]
    want = _host(samples, dict_size, k, d)
    got = cuda_zstd.Dictionary.train(_dev_tensors(samples), dict_size, k, d).content()
    print(name, "host", len(want), "device", len(got))
    assert 256 <= len(want) <= dict_size
    assert got == want
    rc, c = _c_device(samples, dict_size, k, d)
    assert rc == 0 and c == want


def test_constant_byte_exits_by_zero_run():
    samples, dict_size, k, d = _rows()["50x2000_constant"]
    rc, c = _c_device(samples, dict_size, k, d)
    assert rc == 0 and len(c) == 1024 and c == _host(samples, dict_size, k, d)  # one segment, then only zero scores


def test_corpus_shorter_than_k_is_empty():
    import cuda_zstd

    samples = _json(13, [1023])
    with pytest.raises(cuda_zstd.ZstdError):
        _host(samples, 256, 1024, 8)  # the host entry's NULL
    rc, c = _c_device(samples, 256, 1024, 8)
    assert rc == 12 and c is None
    with pytest.raises(cuda_zstd.ZstdError) as e:
        cuda_zstd.Dictionary.train(_dev_tensors(samples), 256, 1024, 8)
    assert e.value.code == 12


def test_2d_tensor_in_place_and_default_parameters():
    import cuda_zstd
    import torch

    samples, dict_size, _, _ = _rows()["40x4096_dict64k"]
    t = torch.from_numpy(np.stack(samples)).cuda()
    assert cuda_zstd.Dictionary.train(t, dict_size).content() == _host(samples, dict_size)
    # a non-contiguous view (every second row) is gathered
    assert cuda_zstd.Dictionary.train(t[::2], 8192).content() == _host(samples[::2], 8192)


@pytest.mark.parametrize("k", [64, 1024])
def test_look_back_edges(k):
    """A 16-byte marker planted at distances seg - 1, seg and seg + 1 from its previous copy: the
    prevdist window and the lo clamp, off by one in each direction."""
    import cuda_zstd

    seg = k - 8 + 1
    a = T.gen(T.DG_RANDOM, 1, 0x5EED0D1D, 8192).copy()
    marker = np.arange(0xA0, 0xB0, dtype=np.uint8)
    pos = [100]
    for dist in (seg - 1, seg, seg + 1, seg - 1, seg + 1, seg):
        pos.append(pos[-1] + max(dist, 16))
    assert pos[-1] + 16 <= len(a)
    for p in pos:
        a[p:p + 16] = marker
    want = _host([a], 4096, k, 8)
    assert cuda_zstd.Dictionary.train(_dev_tensors([a]), 4096, k, 8).content() == want


@pytest.mark.parametrize("k", [64, 1024])
def test_tile_edges(k):
    """300 KiB + 77 bytes: several tiles of every kernel, with an odd remainder."""
    import cuda_zstd

    samples = _json(21, [4096] * 75 + [77])
    want = _host(samples, 16384, k, 8)
    assert cuda_zstd.Dictionary.train(_dev_tensors(samples), 16384, k, 8).content() == want


def test_stream_order():
    """The samples are still being written by a copy queued on the same stream when train is called."""
    import cuda_zstd
    import torch

    samples, dict_size, k, d = _rows()["40x4096_dict64k"]
    staging = torch.from_numpy(np.stack(samples)).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.zeros_like(staging)
        t.copy_(staging, non_blocking=True)
        got = cuda_zstd.Dictionary.train(t, dict_size, k, d, stream=s).content()
    assert got == _host(samples, dict_size, k, d)


def test_temp_and_argument_errors():
    import cuda_zstd
    import torch

    L = cuda_zstd.lib()
    samples, dict_size, k, d = _rows()["64x300"]
    rc, c = _c_device(samples, dict_size, k, d, short_by=1)
    assert rc == 7 and c is None
    flat = torch.from_numpy(np.concatenate(samples)).cuda()
    n = len(samples)
    sizes = (ctypes.c_size_t * n)(*[len(s) for s in samples])
    zeros = (ctypes.c_size_t * n)()
    temp = torch.empty(L.cuda_zstd_train_dictionary_device_get_temp_size(flat.numel(), n, dict_size, k), dtype=torch.uint8, device="cuda")

    def call(szs, num, dsize):
        h = ctypes.c_void_p(1)
        rc = L.cuda_zstd_train_dictionary_device(flat.data_ptr(), szs, num, dsize, k, d, temp.data_ptr(), temp.numel(), None, ctypes.byref(h))
        return rc, h.value

    assert call(zeros, n, dict_size) == (2, None)  # 0 bytes in all
    assert call(sizes, 0, dict_size) == (2, None)
    assert call(None, n, dict_size) == (2, None)
    assert call(sizes, n, 100) == (2, None)
    assert call(sizes, n, 128 * 1024 + 1) == (2, None)
    rc, h = call(sizes, n, dict_size)
    assert rc == 0 and cuda_zstd.Dictionary(h).content() == _host(samples, dict_size, k, d)


def test_end_to_end_device_trained_dictionary(libzstd):
    import cuda_zstd
    import torch

    recs = _cut(T.gen(T.DG_JSON, 256, 0x5EED0D1E, 4096), [4096] * 256)
    d = cuda_zstd.Dictionary.train(torch.from_numpy(np.stack(recs)).cuda(), 16384)
    content = d.content()
    assert content == _host(recs, 16384)
    others = _cut(T.gen(T.DG_JSON, 32, 0x5EED0D1F, 4096), [4096] * 32)
    m = cuda_zstd.Manager(3)
    m.set_dictionary(d)
    outs = m.compress_batch([torch.from_numpy(r.copy()).cuda() for r in others])
    torch.cuda.synchronize()
    for r, o in zip(others, outs):
        f = o.cpu().numpy().tobytes()
        assert f == T.oracle_frame(r, dictionary=content)
        assert T.zstd_decompress(f, len(r), dictionary=content) == r.tobytes()


def test_cpp_surface(tmp_path):
    """dictionary::train_dictionary / create_dictionary_from_samples with device samples
    (tests/cpp_train/dict_train.cpp): contiguous and gathered, use_gpu on and off, a device
    dict_buffer -- all byte-equal to the host-pointer call.  A child process with a timeout."""
    assert os.path.exists(DRIVER), "tests/cpp_train/dict_train not built (__graft_entry__.build())"
    samples, dict_size, _, _ = _rows()["200_ragged_1_5000"]
    (tmp_path / "in.bin").write_bytes(b"".join(s.tobytes() for s in samples))
    (tmp_path / "sizes.bin").write_bytes(np.array([len(s) for s in samples], np.uint64).tobytes())
    r = subprocess.run([DRIVER, str(tmp_path), str(dict_size)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"dict_train: rc {r.returncode}\n{r.stdout}\n{r.stderr}"
    want = _host(samples, dict_size)
    got = (tmp_path / "dict.bin").read_bytes()
    assert len(got) == dict_size and got[dict_size - len(want):] == want and not any(got[:dict_size - len(want)])

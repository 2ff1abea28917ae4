"""The Python surface of dictionary sets: DictionarySet, compress_batch_dicts / decompress_batch_dicts
over host bytes and CUDA tensors.  The kernels' own tests are tests/test_gpu_dictset.py."""
import functools

import numpy as np
import pytest

import zh_testlib as T

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def dict_bytes():
    a = T.gen(T.DG_JSON, 256, 0x5EED0E00, 4096)
    b = T.gen(T.DG_TEXT, 256, 0x5EED0E01, 4096)
    return [T.zdict_train([a[i:i + 4096] for i in range(0, len(a), 4096)], 8192),
            T.gen(T.DG_TEXT, 1, 0x5EED0E02, 3000).tobytes(),  # raw content
            T.zdict_train([b[i:i + 4096] for i in range(0, len(b), 4096)], 8192)]


def test_round_trip_hosts_and_tensors(libzstd):
    import torch

    import cuda_zstd

    ds = dict_bytes()
    s = cuda_zstd.DictionarySet([cuda_zstd.Dictionary.load(d) for d in ds])
    assert len(s) == 3
    kinds = [T.DG_JSON, T.DG_TEXT, T.DG_TEXT, T.DG_JSON]
    idx = [0, 1, 2, -1, 2, 0, 1]
    chunks = [T.gen(kinds[k % 4], 1, 0x5EED0E10 + k, 500 + 4001 * k) for k in range(len(idx))]
    host = cuda_zstd.compress_batch_dicts([c.tobytes() for c in chunks], s, idx, level=3)
    for c, e, f in zip(chunks, idx, host):
        assert isinstance(f, bytes)
        assert T.zstd_decompress(f, len(c), dictionary=ds[e] if e >= 0 else None) == c.tobytes()
    dev = cuda_zstd.compress_batch_dicts([torch.from_numpy(c).cuda() for c in chunks], s, idx, level=3)
    assert [f.cpu().numpy().tobytes() for f in dev] == host
    # raw-content frames carry no ID: they are named by index; the others resolve by ID
    assert cuda_zstd.decompress_batch_dicts(host, s, idx) == [c.tobytes() for c in chunks]
    by_id = [k for k, e in enumerate(idx) if e != 1]
    back = cuda_zstd.decompress_batch_dicts([dev[k] for k in by_id], s)
    assert [b.cpu().numpy().tobytes() for b in back] == [chunks[k].tobytes() for k in by_id]
    small = cuda_zstd.compress_batch_dicts([c.tobytes() for c in chunks], s, idx, level=3, checksum=True, dict_entropy=True)
    assert cuda_zstd.decompress_batch_dicts(small, s, idx, capacities=[len(c) for c in chunks]) == [c.tobytes() for c in chunks]
    assert cuda_zstd.compress_batch_dicts([], s, []) == [] and cuda_zstd.decompress_batch_dicts([], s) == []
    with pytest.raises(cuda_zstd.ZstdError):
        cuda_zstd.compress_batch_dicts([chunks[0].tobytes()], s, [3])  # an index past the set
    s.close()


def test_find_and_duplicates(libzstd):
    import cuda_zstd

    ds = dict_bytes()
    dicts = [cuda_zstd.Dictionary.load(d) for d in ds]
    s = cuda_zstd.DictionarySet(dicts)
    ids = [d.layout()[0] for d in dicts]
    assert ids[1] == 0 and ids[0] and ids[2] and ids[0] != ids[2]
    assert s.find(ids[0]) == 0 and s.find(ids[2]) == 2
    assert s.find(0) == -1 and s.find(ids[0] ^ 1) == -1
    for d in dicts:
        d.close()  # the set copied what it needs
    assert s.find(ids[2]) == 2 and len(s) == 3
    again = [cuda_zstd.Dictionary.load(d) for d in (ds[0], ds[1], ds[1], ds[0])]
    with pytest.raises(cuda_zstd.ZstdError) as e:  # the same non-zero ID twice
        cuda_zstd.DictionarySet(again)
    assert e.value.code == 2
    assert len(cuda_zstd.DictionarySet(again[:3])) == 3  # raw content twice is fine
    with pytest.raises(cuda_zstd.ZstdError):
        cuda_zstd.DictionarySet([])

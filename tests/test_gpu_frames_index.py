"""The frame index (cuda_zstd_seekable_index, zh_frames.hip) on the MI355X: the seek table of
concatenated frames that carry none, against the Python model (zh_frames_model.py, itself pinned
to libzstd by test_frames_model.py).

Every case runs on both paths -- auto (the speculative index unless the candidates overflow) and
the forced serial walker -- and the two must agree byte for byte: return code, *num_frames,
*error_offset and the whole sentinel-filled table buffer."""
import ctypes
import struct

import numpy as np
import pytest

import zh_frames_model as F
import zh_size_model as M
import zh_testlib as T

pytestmark = pytest.mark.gpu

SENT = 0xC3
SLACK = 64  # sentinel bytes behind the table's capacity


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    assert T.zstd() is not None, "the vectors are built with libzstd"
    return torch


@pytest.fixture(scope="module")
def cz(torch_cuda):
    import cuda_zstd

    yield cuda_zstd
    cuda_zstd.lib().cuda_zstd_hip_frames_index_path(0)


def call(torch, cz, stream, path, max_frames=None, capacity=None, temp_short=0, handle=None, in_place=False, shift=0):
    """One call -> (rc, num_frames, error_offset, table_bytes, the table buffer's bytes, path taken).
    shift: the stream starts that many bytes into its allocation (an unaligned pointer)."""
    L = cz.lib()
    size = len(stream)
    n = len(F.walk(stream).frames) + 3 if max_frames is None else max_frames
    cap = 17 + 8 * n if capacity is None else capacity
    buf = torch.full((shift + size + cap + SLACK,), SENT, dtype=torch.uint8, device="cuda")
    buf[shift:shift + size] = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda()
    tab = buf[shift + size:] if in_place else torch.full((cap + SLACK,), SENT, dtype=torch.uint8, device="cuda")
    need = L.cuda_zstd_seekable_index_get_temp_size(size, n)
    temp = torch.empty(need - temp_short, dtype=torch.uint8, device="cuda")
    tb, nf, eo = ctypes.c_size_t(99), ctypes.c_size_t(99), ctypes.c_ulonglong(99)
    L.cuda_zstd_hip_frames_index_path(path)
    try:
        rc = L.cuda_zstd_seekable_index(handle, buf.data_ptr() + shift, size, n, tab.data_ptr(), cap, ctypes.byref(tb), ctypes.byref(nf),
                                        ctypes.byref(eo), temp.data_ptr(), temp.numel(), torch.cuda.current_stream().cuda_stream)
        took = L.cuda_zstd_hip_frames_index_last_path()
    finally:
        L.cuda_zstd_hip_frames_index_path(0)
    torch.cuda.synchronize()
    assert buf[shift:shift + size].cpu().numpy().tobytes() == stream, "the stream was written to"
    return rc, nf.value, eo.value, tb.value, tab[:cap + SLACK].cpu().numpy().tobytes(), took


def both(torch, cz, stream, want, expect_path=0, **kw):
    """Both paths against the model's Index `want`; -> the auto path's result."""
    res = []
    for path in (0, 1):
        rc, nf, eo, tb, tab, took = call(torch, cz, stream, path, **kw)
        assert took == (1 if path else expect_path)
        assert (rc, nf, eo) == (want.rc, want.num_frames, want.error_offset), (path, rc, nf, eo, want[:3])
        assert tb == len(want.table) and tab[:tb] == want.table
        assert tab[tb:] == bytes([SENT]) * (len(tab) - tb), "bytes past the table (or of a failed call's table) were written"
        res.append((rc, nf, eo, tb, tab))
    assert res[0] == res[1]
    return res[0]


# ---- header and block variety -------------------------------------------------------------------
def test_variety(torch_cuda, cz):
    stream, content = F.variety_stream()
    want = F.index(stream)
    assert want.rc == 0 and want.num_frames == len(F.variety()) + 20
    both(torch_cuda, cz, stream, want)
    both(torch_cuda, cz, stream, want, in_place=True)
    # every frame kind once more in front of an unaligned pointer
    both(torch_cuda, cz, stream, want, shift=5)


def test_variety_decodes(torch_cuda, cz):
    stream, content = F.variety_stream()
    assert cz.decompress_frames(stream) == content == T.zstd_decompress(stream, len(content))


# ---- tile edges ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _, _ in F.tile_edge_streams()] if T.zstd() else [])
def test_tile_edges(torch_cuda, cz, name):
    stream = next(s for n, s, _ in F.tile_edge_streams() if n == name)
    want = F.index(stream)
    assert want.rc == 0
    both(torch_cuda, cz, stream, want)


@pytest.mark.parametrize("shift", [1, 3, 13, 15])
def test_tile_edges_unaligned(torch_cuda, cz, shift):
    """An unaligned stream pointer shifts the tiles: the same starts meet other lane edges."""
    name, stream, _ = F.tile_edge_streams()[-1]
    both(torch_cuda, cz, stream, F.index(stream), shift=shift)


# ---- false candidates ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _, _ in F.false_candidate_streams() + F.end_magic_streams()] if T.zstd() else [])
def test_false_candidates(torch_cuda, cz, name):
    stream, content = next((s, c) for n, s, c in F.false_candidate_streams() + F.end_magic_streams() if n == name)
    want = F.index(stream)
    assert want.rc == 0
    # the stream holds more magics than frames, and none of the others made it into the table
    found = sum(stream.count(m) for m in F.magics())
    assert found > want.num_frames or name.startswith("magic_tail")
    both(torch_cuda, cz, stream, want)
    assert cz.decompress_frames(stream) == content


# ---- candidate overflow -------------------------------------------------------------------------
def test_candidate_overflow_takes_the_walker(torch_cuda, cz):
    d = F.text(700, 51)
    f = T.zstd_compress(d)
    max_frames = 4
    payload = b"".join(F.magics()) * 70  # 1,190 magics: more than the 1,032 candidates max_frames = 4 admits
    assert len(payload) // 4 > F.candidates(max_frames) == 2 * max_frames + 1024
    stream = f + F.hand_frame(payload, single=True) + F.skippable(b"s") + f
    want = F.index(stream, max_frames=max_frames)
    assert want.rc == 0 and want.num_frames == 4
    both(torch_cuda, cz, stream, want, expect_path=1, max_frames=max_frames)
    # with room for the candidates the speculative index takes it (and max_frames one short is 7 on both)
    both(torch_cuda, cz, stream, F.index(stream, max_frames=100), expect_path=0, max_frames=100)
    both(torch_cuda, cz, stream, F.index(stream, max_frames=3), expect_path=1, max_frames=3)


# ---- doubling rounds ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 5000])
def test_frame_counts(torch_cuda, cz, n):
    stream, content = next((s, c) for k, s, c in F.count_streams() if k == n)
    want = F.index(stream)
    assert want.rc == 0 and want.num_frames == n
    both(torch_cuda, cz, stream, want)
    if n in (65, 5000):
        assert cz.decompress_frames(stream) == content


# ---- malformed streams --------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in F.malformed_streams()] if T.zstd() else [])
def test_malformed(torch_cuda, cz, name):
    stream = next(s for n, s in F.malformed_streams() if n == name)
    want = F.index(stream)
    assert want.rc in (1, 6) and (want.rc == 1) == (name == "wrong_first_magic") and want.table == b""
    both(torch_cuda, cz, stream, want, max_frames=8)


def test_python_error_carries_the_report(torch_cuda, cz):
    name, stream = next(v for v in F.malformed_streams() if v[0] == "garbage_3")
    want = F.index(stream)
    with pytest.raises(cz.ZstdError) as e:
        cz.seekable_index(stream)
    assert (e.value.code, e.value.num_frames, e.value.error_offset) == (cz.CORRUPT, want.num_frames, want.error_offset)


# ---- capacities and arguments -------------------------------------------------------------------
def test_capacities(torch_cuda, cz):
    n, stream, _ = F.count_streams()[5]
    assert n == 65
    full = F.index(stream)
    both(torch_cuda, cz, stream, full, max_frames=65, capacity=17 + 8 * 65)  # exactly enough of both
    both(torch_cuda, cz, stream, F.Index(F.TOO_SMALL, 65, 0, b""), max_frames=64)
    assert F.index(stream, max_frames=64) == F.Index(F.TOO_SMALL, 65, 0, b"")
    both(torch_cuda, cz, stream, F.Index(F.TOO_SMALL, 65, 0, b""), max_frames=65, capacity=17 + 8 * 65 - 1)
    assert F.index(stream, table_capacity=17 + 8 * 65 - 1) == F.Index(F.TOO_SMALL, 65, 0, b"")
    # temp one byte short: nothing is launched, nothing is reported
    for path in (0, 1):
        rc, nf, eo, tb, tab, _ = call(torch_cuda, cz, stream, path, temp_short=1)
        assert (rc, nf, eo, tb) == (F.TOO_SMALL, 0, 0, 0) and tab == bytes([SENT]) * len(tab)


def test_arguments(torch_cuda, cz):
    L = cz.lib()
    t = torch_cuda.full((4096,), SENT, dtype=torch_cuda.uint8, device="cuda")
    tb, nf, eo = ctypes.c_size_t(9), ctypes.c_size_t(9), ctypes.c_ulonglong(9)
    ok = dict(h=None, s=t.data_ptr(), size=9, n=4, tab=t.data_ptr() + 1024, cap=100, tb=ctypes.byref(tb), nf=ctypes.byref(nf), eo=ctypes.byref(eo),
              temp=t.data_ptr() + 2048)
    for bad in (dict(s=None), dict(size=0), dict(tab=None), dict(tb=None), dict(nf=None), dict(eo=None)):
        a = dict(ok, **bad)
        rc = L.cuda_zstd_seekable_index(a["h"], a["s"], a["size"], a["n"], a["tab"], a["cap"], a["tb"], a["nf"], a["eo"], a["temp"], 1 << 30, None)
        assert rc == F.INVALID, bad
    torch_cuda.cuda.synchronize()
    assert bool((t == SENT).all())


def test_python_guesses_max_frames(torch_cuda, cz):
    """5,000 frames in 44 KiB: the first guess is too low, the second call has the count."""
    n, stream, content = F.count_streams()[-1]
    out = cz.seekable_index(stream)
    want = F.index(stream)
    assert out.cpu().numpy().tobytes() == stream + want.table
    r = cz.SeekableReader(out)
    assert r.num_frames == n and r.size == len(content)


# ---- end to end ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(torch_cuda):
    """~40 frames: sized and size-less, checksummed, empty, raw, multi-block, skippable between."""
    rng = np.random.default_rng(77)
    parts, chunks = [], []
    for i in range(34):
        n = int(rng.integers(1, 30000))
        d = F.text(n, 100 + i) if i % 5 else F.noise(n, 100 + i)
        parts.append(T.zstd_compress(d, checksum=bool(i % 2), content_size=bool(i % 3)))
        chunks.append(d)
        if i % 6 == 0:
            parts.append(F.skippable(b"k" * (i % 4), i % 16))
            chunks.append(b"")
        if i % 11 == 3:
            parts.append(F.EMPTY)
            chunks.append(b"")
    d = F.text(200000, 999)
    parts.append(T.zstd_compress(d, content_size=False))
    chunks.append(d)
    assert 40 <= len(parts) <= 48
    return b"".join(parts), chunks


def test_decompress_frames_mixed(torch_cuda, cz, mixed):
    stream, chunks = mixed
    content = b"".join(chunks)
    want = F.index(stream)
    assert want.rc == 0 and want.num_frames == len(chunks)
    both(torch_cuda, cz, stream, want)
    assert T.zstd_decompress(stream, len(content)) == content
    assert cz.decompress_frames(stream) == content
    dev = torch_cuda.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda()
    got = cz.decompress_frames(dev)
    assert got.is_cuda and got.cpu().numpy().tobytes() == content
    assert cz.Manager(3).decompress(stream, capacity=len(content)) == content  # the one-item route it replaces
    # stock zstd reads stream + table as a stream too
    assert T.zstd_decompress(cz.seekable_index(stream).cpu().numpy().tobytes(), len(content)) == content


def test_read_ranges(torch_cuda, cz, mixed):
    stream, chunks = mixed
    content = b"".join(chunks)
    starts = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).tolist()
    w = F.walk(stream)
    skip = next(i for i, f in enumerate(w.frames) if f.skippable and 0 < i < len(chunks) - 1)
    sizeless = next(i for i, f in enumerate(w.frames) if not f.skippable and f.fcs is None and len(chunks[i]) > 500)
    ranges = [(starts[3] - 7, 20),  # straddles a frame boundary
              (starts[10] - 1, len(chunks[10]) + 2),  # a whole frame and a byte of each neighbour
              (starts[skip], 100),  # starts at a skippable entry (which has no content)
              (starts[sizeless] + 100, 300),  # inside a frame that states no size
              (starts[-2] + 70000, 100000),  # inside the last, multi-block size-less frame
              (0, 1), (len(content) - 1, 1), (len(content), 0)]
    r = cz.SeekableReader.from_frames(stream)
    assert r.num_frames == len(chunks) and r.size == len(content)
    got = r.read_ranges([a for a, _ in ranges], [n for _, n in ranges])
    assert got == [content[a:a + n] for a, n in ranges]
    assert r.read(starts[sizeless], len(chunks[sizeless])) == chunks[sizeless]


def test_sizeless_frame_carries_its_real_size(torch_cuda, cz):
    d = F.text(123457, 61)
    stream = F.EMPTY + T.zstd_compress(d, content_size=False) + F.rle_frame(3, 70001, stated=False)
    rc, nf, eo, tb, tab = both(torch_cuda, cz, stream, F.index(stream))
    assert rc == 0 and [struct.unpack_from("<I", tab, 8 + 8 * i + 4)[0] for i in range(3)] == [0, 123457, 70001]


@pytest.fixture(scope="module")
def dict_case(torch_cuda):
    a = T.gen(T.DG_JSON, 8, 0xD1C7, 8192).tobytes()
    dct = T.zdict_train([a[i:i + 2048] for i in range(0, len(a), 2048)], 8192)
    chunks = [T.gen(T.DG_JSON, 1, 0xD1C8 + i, 3000 + 17 * i).tobytes() for i in range(6)]
    frames = [T.zstd_compress_dict(c, dct) for c in chunks]
    assert all(F.frame_dict_id(f) == T.dict_layout(dct)[0] != 0 for f in frames)
    return dct, chunks, frames


def test_dictionary_frames_with_sizes_need_no_handle(torch_cuda, cz, dict_case):
    dct, chunks, frames = dict_case
    stream = b"".join(frames)
    want = F.index(stream)
    assert want.rc == 0 and want.num_frames == 6
    both(torch_cuda, cz, stream, want)
    dec = cz.BatchedDecompressor()
    dec.set_dictionary(cz.Dictionary.load(dct))
    assert cz.decompress_frames(stream, dec) == b"".join(chunks)


def test_sizeless_dictionary_frame(torch_cuda, cz, dict_case):
    dct, chunks, frames = dict_case
    bare = M.drop_content_size(frames[3])
    stream = frames[0] + F.skippable(b"x") + frames[1] + bare + frames[4]
    # without the dictionary: the decoder's code for a wrong dictionary, at that frame
    want = F.index(stream)
    assert want == F.Index(F.DICT_WRONG, 3, len(frames[0]) + 9 + len(frames[1]), b"")
    both(torch_cuda, cz, stream, want)
    dec = cz.BatchedDecompressor()
    dec.set_dictionary(cz.Dictionary.load(dct))
    want = F.index(stream, dictionary=dct)
    assert want.rc == 0 and struct.unpack_from("<I", want.table, 8 + 8 * 3 + 4)[0] == len(chunks[3])
    both(torch_cuda, cz, stream, want, handle=dec._h)
    assert cz.decompress_frames(stream, dec) == chunks[0] + chunks[1] + chunks[3] + chunks[4]

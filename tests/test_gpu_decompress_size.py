"""The batched on-device decompressed-size query (zh_dec_size_kernel through
cuda_zstd_get_decompressed_sizes_async and nvcomp_zstd_batched_get_decompress_size_async_v5) on the
MI355X, held to the plain model of tests/zh_size_model.py (test_size_model.py checks that model
against known truth on the CPU) and to the decoder itself: for every buffer the decoder accepts, the
query answers exactly the bytes the decoder produces, with or without a Frame_Content_Size."""
import ctypes
import json
import os

import numpy as np
import pytest

import zh_frames as F
import zh_seqframes as S
import zh_size_model as M
import zh_testlib as T

pytestmark = pytest.mark.gpu

A256 = lambda n: (n + 255) // 256 * 256  # noqa: E731
POISON, ST_POISON, MARGIN = 0x5A5A5A5A5A5A5A5A, -7, 32
# status of a rejected buffer by entry: the manager's Status values, the nvcomp codes
INVALID = {"manager": 2, "nvcomp": 2}
BAD_MAGIC = {"manager": 5, "nvcomp": 1}
CORRUPT = {"manager": 6, "nvcomp": 6}
DICT_MISMATCH = {"manager": 9, "nvcomp": 1}
ENTRIES = ("manager", "nvcomp")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


class Query:
    """One handle of either entry (with a dictionary, if given) and the raw device-array call."""

    def __init__(self, entry, dictionary=None):
        import cuda_zstd

        self.entry = entry
        self.h = cuda_zstd.Manager(3) if entry == "manager" else cuda_zstd.BatchManager(3)
        if dictionary is not None:
            self.h.set_dictionary(cuda_zstd.Dictionary.load(dictionary))

    def raw(self, ptrs, sizes, n, out, st, stream):
        import cuda_zstd

        L = cuda_zstd.lib()
        if self.entry == "manager":
            return L.cuda_zstd_get_decompressed_sizes_async(self.h._h, ptrs, sizes, n, out, st, stream)
        return L.nvcomp_zstd_batched_get_decompress_size_async_v5(self.h._h, ptrs, sizes, out, st, n, stream)

    def __call__(self, torch, bufs, with_status=True):
        """Sizes and statuses of device buffers (tensors, or (pointer, size) pairs).  The outputs sit
        inside larger poisoned allocations: only the entries of the batch change."""
        n = len(bufs)
        pairs = [b if isinstance(b, tuple) else (b.data_ptr(), b.numel()) for b in bufs]
        i64 = lambda x: torch.tensor(x, dtype=torch.int64, device="cuda")  # noqa: E731
        ptrs, sizes = i64([p for p, _ in pairs]), i64([s for _, s in pairs])
        out = torch.full((n + 2 * MARGIN,), POISON, dtype=torch.int64, device="cuda")
        st = torch.full((n + 2 * MARGIN,), ST_POISON, dtype=torch.int32, device="cuda")
        rc = self.raw(ptrs.data_ptr(), sizes.data_ptr(), n, out.data_ptr() + 8 * MARGIN, st.data_ptr() + 4 * MARGIN if with_status else None,
                      torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        ho, hs = out.cpu().numpy(), st.cpu().numpy()
        assert (ho[:MARGIN] == POISON).all() and (ho[MARGIN + n:] == POISON).all()
        assert (hs[:MARGIN] == ST_POISON).all() and (hs[MARGIN + n:] == ST_POISON).all()
        if not with_status:
            assert (hs == ST_POISON).all()
        return [int(v) for v in ho[MARGIN:MARGIN + n].view(np.uint64)], [int(v) for v in hs[MARGIN:MARGIN + n]]


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


def _dev(torch, b):
    a = np.frombuffer(bytes(b), np.uint8).copy()
    return torch.from_numpy(a if a.size else np.zeros(1, np.uint8)).cuda()[: len(a)]


_model = {}


def model(v, dictionary=None):
    """The model's (size, ok) of a vector, computed once."""
    k = (repr(v), dictionary is not None)
    if k not in _model:
        _model[k] = M.size(v.bytes, dictionary)
    return _model[k]


def _check_vectors(torch, q, vs, total, dictionary=None):
    entries = _entries(vs)
    if total:
        entries = [entries[k % len(entries)] for k in range(total)]
    keep, bufs = _arena(torch, entries)
    sizes, st = q(torch, bufs)
    bad = []
    for k, ((v, a), sz, s) in enumerate(zip(entries, sizes, st)):
        want, ok = model(v, dictionary)
        good = (s == 0) == ok and sz == want
        if v.expect == "nonzero":
            good = good and s == DICT_MISMATCH[q.entry]
        elif not ok:
            good = good and s == CORRUPT[q.entry]
        if v.want is not None and v.expect != "nonzero":
            good = good and s == 0 and sz == len(v.want)
        if not good:
            bad.append((k, repr(v), a, s, sz, want, ok))
    assert not bad, (len(bad), bad[:12])
    return len(entries)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("total", [None, 2304])
def test_sequence_vectors(torch_cuda, entry, total):
    """Every hand-assembled vector, the ones built to be rejected included: status and size are the
    model's, and an accepted vector's size is its decoded length."""
    n = _check_vectors(torch_cuda, Query(entry), S.vectors(), total)
    assert n == total if total else 200 < n < 1024
    assert {model(v)[1] for v in S.vectors() if v.want is None} == {True, False}  # rejects of both kinds


@pytest.mark.parametrize("entry", ENTRIES)
def test_dictionary_vectors(torch_cuda, entry):
    d = S.dictionary()
    _check_vectors(torch_cuda, Query(entry, d), S.dict_vectors(), None, d)


def _zstd_dict_nofcs(data, dictionary, level):
    """libzstd frame of `data` with the dictionary loaded and no Frame_Content_Size (what a
    streaming writer makes): ZSTD_compress2 with contentSizeFlag (200) off."""
    z, vp = T.zstd(), ctypes.c_void_p
    z.ZSTD_createCCtx.restype = vp
    z.ZSTD_freeCCtx.argtypes = [vp]
    z.ZSTD_CCtx_setParameter.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    z.ZSTD_CCtx_setParameter.restype = ctypes.c_size_t
    z.ZSTD_CCtx_loadDictionary.argtypes = [vp, vp, ctypes.c_size_t]
    z.ZSTD_CCtx_loadDictionary.restype = ctypes.c_size_t
    z.ZSTD_compress2.argtypes = [vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t]
    z.ZSTD_compress2.restype = ctypes.c_size_t
    src, dd = np.frombuffer(bytes(data), np.uint8).copy(), np.frombuffer(bytes(dictionary), np.uint8).copy()
    c = z.ZSTD_createCCtx()
    assert not z.ZSTD_isError(z.ZSTD_CCtx_setParameter(c, 100, level)) and not z.ZSTD_isError(z.ZSTD_CCtx_setParameter(c, 200, 0))
    assert not z.ZSTD_isError(z.ZSTD_CCtx_loadDictionary(c, dd.ctypes.data, len(dd)))
    out = np.zeros(len(src) + 1024, np.uint8)
    r = z.ZSTD_compress2(c, out.ctypes.data, len(out), src.ctypes.data, len(src))
    z.ZSTD_freeCCtx(c)
    assert not z.ZSTD_isError(r)
    return out[:r].tobytes()


def _hand_dict_frame():
    """A formatted dictionary with tables of its own (zh_dict_entropy.make_dict) and a frame without a
    content size whose only block repeats all three of them."""
    import zh_dict_entropy as DE

    ll, of, ml = (S._fse_norm(s, lg)[1:] for s, lg in (([4, 9], 6), ([2, 3], 5), ([2, 6], 7)))
    d = DE.make_dict(S._rng("size_dict").integers(0, 256, 4096, dtype=np.uint8).tobytes(), {65: 1, 66: 2, 67: 2}, of=of, ml=ml, ll=ll, dict_id=0x4242)
    blk = S._block("size_dict_blk", [(4, 5, 6), (9, 9, 9)], 1, modes=("repeat",) * 3)
    body = S._block_bytes(blk, True, [S.Table(S.fse_cells(list(n), lg), lg) for n, lg in (ll, of, ml)])
    frame = S.MAGIC.to_bytes(4, "little") + bytes([0x02, 0x00]) + (0x4242).to_bytes(2, "little") + body
    return d, frame, S._claimed_size(S.frame([blk]))


@pytest.mark.parametrize("entry", ENTRIES)
def test_formatted_dictionary(torch_cuda, entry, libzstd):
    """Frames without a content size whose first block takes its tables from a formatted
    dictionary (Repeat_Mode, treeless literals): sized with the dictionary, an error without."""
    torch = torch_cuda
    a = T.gen(T.DG_JSON, 512, 0x5EED0005, 4096)
    zd = T.zdict_train([a[i:i + 4096] for i in range(0, len(a), 4096)], 16384)
    rec = T.gen(T.DG_JSON, 1, 0x5EED0A05, 70000)
    cases = [(zd, _zstd_dict_nofcs(rec[:n], zd, lv), n) for n in (500, 3000, 20000, 70000) for lv in (1, 3, 19)]
    firsts = [F.walk(f)[0] for _, f, _ in cases]
    assert all(not b["fcs"] for b in firsts)
    assert any("repeat" in b.get("modes", ()) for b in firsts) and any(b.get("lit") == "treeless" for b in firsts)
    hd, hframe, hsize = _hand_dict_frame()
    for d, group in ((zd, cases), (hd, [(hd, hframe, hsize)])):
        bufs = [_dev(torch, f) for _, f, _ in group]
        want = [n for _, _, n in group]
        assert [M.size(f, d) for _, f, _ in group] == [(n, True) for n in want]
        q = Query(entry, d)
        assert q(torch, bufs) == (want, [0] * len(group))
        # the decoder agrees
        import cuda_zstd

        m = cuda_zstd.Manager(3)
        m.set_dictionary(cuda_zstd.Dictionary.load(d))
        outs, st = m.decompress_batch(bufs, [n + 64 for n in want], raise_on_error=False)
        assert st == [0] * len(group) and [o.numel() for o in outs] == want
        sizes, st = Query(entry)(torch, bufs)
        assert sizes == [0] * len(group) and all(s == DICT_MISMATCH[entry] for s in st)


def _libzstd_nofcs():
    text = T.gen(T.DG_TEXT, 1, 5, 200000).tobytes()
    out = []
    for lv in (1, 3, 19):
        out.append((f"text_200000_l{lv}_nofcs", T.zstd_compress(text, lv, content_size=False), text))
        out.append((f"zeros_300000_l{lv}_nofcs", T.zstd_compress(bytes(300000), lv, content_size=False), bytes(300000)))
    return out


def _golden():
    vecs = json.load(open(os.path.join(T.GOLDEN, "decode_frames.json")))["vectors"]
    return [(v["name"], bytes.fromhex(v["frame"]), v["size"]) for v in vecs if "expect_error" not in v]


@pytest.mark.parametrize("entry", ENTRIES)
def test_golden_and_libzstd_frames(torch_cuda, entry, libzstd):
    torch = torch_cuda
    gold, lz = _golden(), _libzstd_nofcs()
    dropped = [(n + "_dropped", M.drop_content_size(f), s) for n, f, s in gold if M.drop_content_size(f) is not None]
    group = gold + dropped + [(n, f, len(w)) for n, f, w in lz]
    assert any(len(w) > 16 * len(f) for _, f, w in lz)  # where 16x the input is no capacity
    sizes, st = Query(entry)(torch, [_dev(torch, f) for _, f, _ in group])
    bad = [(n, s, c, want) for (n, _, want), s, c in zip(group, sizes, st) if c != 0 or s != want]
    assert not bad, bad[:10]


def test_decompress_without_capacity(torch_cuda, libzstd):
    """Manager.decompress and decompress_batch take their capacities from the query: frames without
    a content size come back whole, the zeros (ratio 10,000) included."""
    import cuda_zstd

    torch = torch_cuda
    lz = _libzstd_nofcs()
    m = cuda_zstd.Manager(3)
    for name, f, want in lz[:2] + lz[-1:]:
        assert m.decompress(_dev(torch, f)).cpu().numpy().tobytes() == want, name
        assert m.decompress(f) == want, name  # host bytes in, bytes out
    outs = m.decompress_batch([_dev(torch, f) for _, f, _ in lz])
    assert [o.cpu().numpy().tobytes() for o in outs] == [w for _, _, w in lz]
    assert cuda_zstd.decompressed_sizes([f for _, f, _ in lz]) == [len(w) for _, _, w in lz]
    assert m.decompressed_sizes([_dev(torch, f) for _, f, _ in lz], raise_on_error=False) == ([len(w) for _, _, w in lz], [0] * len(lz))


@pytest.mark.parametrize("entry", ENTRIES)
def test_hand_made_and_bad_items(torch_cuda, entry):
    """The CPU test's hand-made buffers (concatenations, skippable frames, raw / RLE only, an
    8-byte content size of 2^40), then a batch with an empty, a bad-magic and a truncated item
    among valid ones: each bad item has its own status and size 0, the neighbours their sizes."""
    torch = torch_cuda
    hm = M.hand_made()
    q = Query(entry)
    sizes, st = q(torch, [_dev(torch, d) for _, d, _, _ in hm])
    assert sizes == [w for _, _, w, _ in hm] and st == [0] * len(hm)
    assert max(sizes) > 1 << 40
    good = [d for _, d, _, ok in hm if ok]
    gsize = [w for _, _, w, ok in hm if ok]
    magic = bytes([good[1][0] ^ 0x40]) + good[1][1:]
    keep = [_dev(torch, b) for b in (good[0], magic, good[1], good[2][:-1], good[2], good[3][:7])]
    bufs = [(keep[0].data_ptr(), 0)] + keep + [(0, 100), (0, 0)]
    sizes, st = q(torch, bufs)
    assert sizes == [0, gsize[0], 0, gsize[1], 0, gsize[2], 0, 0, 0]
    assert st == [INVALID[entry], 0, BAD_MAGIC[entry], 0, CORRUPT[entry], 0, CORRUPT[entry], INVALID[entry], INVALID[entry]]
    # the sum of the frames' sizes leaves 64 bits
    big = [d for n, d, _, _ in hm if n == "fcs_2_40"][0]
    top = big[:5] + ((1 << 64) - 2).to_bytes(8, "little") + big[13:]
    sizes, st = q(torch, [_dev(torch, top), _dev(torch, top + top), _dev(torch, top + good[3])])
    assert sizes == [(1 << 64) - 2, 0, 0] and st == [0, CORRUPT[entry], CORRUPT[entry]]


@pytest.mark.parametrize("entry", ENTRIES)
def test_output_discipline(torch_cuda, entry):
    """Only the batch's entries of the two output arrays change (Query checks the poison around
    them on every call); a null status array works; count 0 touches nothing and needs no arrays."""
    torch = torch_cuda
    hm = M.hand_made()
    q = Query(entry)
    bufs = [_dev(torch, d) for _, d, _, _ in hm]
    sizes, st = q(torch, bufs, with_status=False)
    assert sizes == [w for _, _, w, _ in hm] and st == [ST_POISON] * len(hm)
    out = torch.full((8,), POISON, dtype=torch.int64, device="cuda")
    stt = torch.full((8,), ST_POISON, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert q.raw(None, None, 0, out.data_ptr(), stt.data_ptr(), s) == 0
    assert q.raw(None, None, 0, None, None, s) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == POISON).all() and (stt.cpu().numpy() == ST_POISON).all()
    assert q.raw(None, None, 3, out.data_ptr(), stt.data_ptr(), s) == 2  # null arrays with a count: refused, nothing launched


def test_consistent_with_decode(torch_cuda, libzstd):
    """For every buffer of this file that the decoder accepts when given a generous capacity, the
    query's size is the decoder's out_sizes -- and wherever the query reports an error, so does the
    decoder."""
    import cuda_zstd

    torch = torch_cuda
    plain = [(repr(v), v.bytes) for v in S.vectors()] + [(n, f) for n, f, _ in _golden()] + [(n, f) for n, f, _ in _libzstd_nofcs()]
    plain += [(n, d) for n, d, _, ok in M.hand_made() if ok]
    plain += [(n + "_dropped", M.drop_content_size(f)) for n, f, _ in _golden() if M.drop_content_size(f) is not None]
    d = S.dictionary()
    accepted = 0
    for dictionary, group in ((None, plain), (d, [(repr(v), v.bytes) for v in S.dict_vectors()])):
        m = cuda_zstd.Manager(3)
        if dictionary is not None:
            m.set_dictionary(cuda_zstd.Dictionary.load(dictionary))
        bufs = [_dev(torch, f) for _, f in group]
        sizes, st = m.decompressed_sizes(bufs, raise_on_error=False)
        caps = [max(M.size(f, dictionary)[0], 4 * len(f)) + 4096 for _, f in group]
        outs, dst = m.decompress_batch(bufs, caps, raise_on_error=False)
        bad = []
        for (name, _), sz, s, o, ds in zip(group, sizes, st, outs, dst):
            if ds == 0:
                accepted += 1
                if s != 0 or sz != o.numel():
                    bad.append((name, sz, s, o.numel()))
            if s != 0 and ds == 0:
                bad.append((name, "the query rejects what the decoder accepts", s))
        assert not bad, bad[:10]
    # every buffer here that is valid decoded: all but the vectors built to be rejected
    rejected = sum(1 for v in S.vectors() + S.dict_vectors() if v.want is None or v.expect == "nonzero")
    assert accepted == len(plain) + len(S.dict_vectors()) - rejected and rejected >= 10


def test_stream_order(torch_cuda):
    """Compress a small batch, then size the outputs on the same stream from the device size array
    the compressor wrote, nothing synchronised between the two calls."""
    import cuda_zstd

    torch = torch_cuda
    lens = [1, 100, 4097, 65536, 30000, 12345, 65535, 2]
    src = T.gen(T.DG_TEXT, len(lens), 0x5EED0B01, 65536)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev = torch.from_numpy(src).cuda()
        bc, bd = cuda_zstd.BatchManager(3, 65536), cuda_zstd.BatchedDecompressor()
        n, slot = len(lens), A256(bc.max_out(65536))
        i64 = lambda x: torch.tensor(x, dtype=torch.int64, device="cuda")  # noqa: E731
        ob = torch.empty(n * slot, dtype=torch.uint8, device="cuda")
        in_ptrs, in_sizes = dev.data_ptr() + torch.arange(n, dtype=torch.int64, device="cuda") * 65536, i64(lens)
        out_ptrs = ob.data_ptr() + torch.arange(n, dtype=torch.int64, device="cuda") * slot
        osz, cst = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        qsz, qst = torch.full((n,), -1, dtype=torch.int64, device="cuda"), torch.full((n,), -1, dtype=torch.int32, device="cuda")
        temp = torch.empty(bc.temp_size(n, 65536), dtype=torch.uint8, device="cuda")
        bc.compress_async(in_ptrs, in_sizes, 65536, out_ptrs, osz, cst, temp, stream=s)
        bd.get_sizes_async(out_ptrs, osz, qsz, qst, stream=s)
    s.synchronize()
    assert cst.tolist() == [0] * n and qst.tolist() == [0] * n and qsz.tolist() == lens


def test_python_plumbing(torch_cuda):
    """decompress_batch of 512 small frames without capacities: one size launch in place of a
    header copy per frame.  A corrupt frame among them keeps the fallback capacity, and the
    decoder's status for it is what the caller sees; the others decode."""
    import cuda_zstd

    torch = torch_cuda
    m = cuda_zstd.Manager(3)
    src = T.gen(T.DG_JSON, 512, 0x5EED0B02, 2048)
    recs = [src[i * 2048:i * 2048 + 1 + (i * 37) % 2048] for i in range(512)]
    frames = m.compress_batch([torch.from_numpy(r.copy()).cuda() for r in recs])
    torch.cuda.synchronize()
    outs = m.decompress_batch(frames)
    assert [o.cpu().numpy().tobytes() for o in outs] == [r.tobytes() for r in recs]
    assert m.decompressed_sizes(frames) == [len(r) for r in recs]
    k = 300
    broken = frames[k][: frames[k].numel() - 3].clone()
    sizes, st = m.decompressed_sizes(frames[:k] + [broken] + frames[k + 1:], raise_on_error=False)
    assert st[k] == 6 and sizes[k] == 0 and sum(1 for s in st if s) == 1
    with pytest.raises(cuda_zstd.ZstdError):
        m.decompressed_sizes([broken])
    outs, st = m.decompress_batch(frames[:k] + [broken] + frames[k + 1:], raise_on_error=False)
    assert st[k] == cuda_zstd.CORRUPT and sum(1 for s in st if s) == 1
    assert all(o.cpu().numpy().tobytes() == r.tobytes() for i, (o, r) in enumerate(zip(outs, recs)) if i != k)
    with pytest.raises(cuda_zstd.ZstdError) as e:
        m.decompress(broken)
    assert e.value.code == cuda_zstd.CORRUPT

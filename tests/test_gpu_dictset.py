"""A batch against a set of dictionaries (cuda_zstd_dict_set_*, nvcomp_zstd_batched_compress_dicts_async_v5,
nvcomp_zstd_batched_decompress_dicts_async_v5 and the ID-resolving decode and size entries; csrc/zh_dictset.h,
zh_plan_kernel, the matchers' and the entropy kernel's per-entry tables, the decoder's frame_dict).

One set of six entries -- raw content of 256, 511 and 512 bytes, two ZDICT-trained formatted
dictionaries (JSON, text) and 128 KiB of raw content -- is built once per module; so are the
single-dictionary handles' frames every set frame is compared with.  Every comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest

import zh_testlib as T

pytestmark = pytest.mark.gpu

SIZES = [1, 15, 16, 4095, 32767, 32768, 32769, 65536]
SENTINEL = 0xA5
INVALID, CORRUPT, DICT_WRONG = 2, 6, 1  # nvcomp-style codes (zh_decode.hip to_nvcomp)
NENT = 6
JSON_D, TEXT_D = 3, 4  # the formatted entries


@functools.lru_cache(maxsize=None)
def entries():
    js = T.gen(T.DG_JSON, 1, 0x5EED0D00, 70000)
    tx = T.gen(T.DG_TEXT, 1, 0x5EED0D01, 70000)
    a = T.gen(T.DG_JSON, 512, 0x5EED0D02, 4096)
    b = T.gen(T.DG_TEXT, 512, 0x5EED0D03, 4096)
    out = [js[:256].tobytes(), tx[:511].tobytes(), js[1000:1512].tobytes(),
           T.zdict_train([a[i:i + 4096] for i in range(0, len(a), 4096)], 16384),
           T.zdict_train([b[i:i + 4096] for i in range(0, len(b), 4096)], 16384),
           np.concatenate([js[:65536], tx[:65536]]).tobytes()]
    ids = [T.dict_layout(e)[0] for e in out]
    assert ids[0] == ids[1] == ids[2] == ids[5] == 0 and ids[3] and ids[4] and ids[3] != ids[4]
    assert [len(e) for e in out[:3]] + [len(out[5])] == [256, 511, 512, 131072]
    return out


@functools.lru_cache(maxsize=None)
def dset():
    import cuda_zstd

    return cuda_zstd.DictionarySet([cuda_zstd.Dictionary.load(e) for e in entries()])


@functools.lru_cache(maxsize=None)
def stream_of(kind, seed, total):
    return T.gen(kind, 1, 0x5EED0D10 + seed, total)


@functools.lru_cache(maxsize=None)
def items(max_chunk):
    """[(chunk, entry index)]: 48 chunks of the grid sizes cut from JSON and text streams, chunk k
    against entry k mod 6, every seventh -1; then one item each with index -2 and 6 put between them."""
    out = []
    for k in range(48):
        n = SIZES[k % 8]
        if n > max_chunk:
            continue
        s = stream_of(T.DG_JSON if (k // 8) % 2 == 0 else T.DG_TEXT, k, 100 + n)
        out.append((s[100:], -1 if k % 7 == 6 else k % NENT))
    out.insert(3, (stream_of(T.DG_JSON, 100, 5000), -2))
    out.insert(10, (stream_of(T.DG_TEXT, 101, 5000), NENT))
    return out


class Arena:
    """Host buffers laid out at odd addresses of one device allocation."""

    def __init__(self, bufs):
        import torch

        self.off, o = [], 1
        for b in bufs:
            self.off.append(o)
            o += len(b) + 2
            o |= 1
        host = np.zeros(o + 256, np.uint8)
        for b, at in zip(bufs, self.off):
            if len(b):
                host[at:at + len(b)] = np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else b
        self.dev = torch.from_numpy(host).cuda()
        base = self.dev.data_ptr()
        assert base % 16 == 0
        self.ptrs = [base + at for at in self.off]
        self.sizes = [len(b) for b in bufs]
        assert all(p % 2 == 1 for p in self.ptrs)


def i64(v):
    import torch

    return torch.tensor(list(v), dtype=torch.int64, device="cuda")


def i32(v):
    import torch

    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def compress(chunks, level, max_chunk, idx=None, dictionary=None, checksum=False, dict_entropy=False, stream=None, arena=None):
    """One call -> (frames, sizes, statuses, raw output slots).  idx: the set route with these entry
    indices; else the plain entry on a handle with `dictionary` (bytes or None) set."""
    import torch

    import cuda_zstd

    n = len(chunks)
    ar = arena or Arena(chunks)
    bc = cuda_zstd.BatchedCompressor(level, 65536, checksum=checksum, dict_entropy=dict_entropy)
    slot = (bc.max_out(max_chunk) + 255) // 256 * 256
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        out = torch.full((n * slot,), SENTINEL, dtype=torch.uint8, device="cuda")
        out_ptrs = i64(out.data_ptr() + i * slot for i in range(n))
        out_sizes = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        if idx is not None:
            bc.set_dictionary_set(dset())
            temp = torch.empty(bc.temp_size_dicts(n, max_chunk), dtype=torch.uint8, device="cuda")
            bc.compress_dicts_async(i64(ar.ptrs), i64(ar.sizes), i32(idx), max_chunk, out_ptrs, out_sizes, status, temp, stream)
        else:
            if dictionary is not None:
                bc.set_dictionary(cuda_zstd.Dictionary.load(dictionary))
            temp = torch.empty(bc.temp_size(n, max_chunk), dtype=torch.uint8, device="cuda")
            bc.compress_async(i64(ar.ptrs), i64(ar.sizes), max_chunk, out_ptrs, out_sizes, status, temp, stream)
    torch.cuda.synchronize()
    bc.close()
    sizes, st, host = out_sizes.cpu().tolist(), status.cpu().tolist(), out.cpu().numpy()
    frames = [host[i * slot:i * slot + max(sizes[i], 0)].tobytes() for i in range(n)]
    return frames, sizes, st, [host[i * slot:(i + 1) * slot] for i in range(n)]


@functools.lru_cache(maxsize=None)
def set_frames(level, max_chunk, checksum=False):
    its = items(max_chunk)
    return compress([c for c, _ in its], level, max_chunk, idx=[e for _, e in its], checksum=checksum)


@functools.lru_cache(maxsize=None)
def single_frames(level, max_chunk, checksum=False, dict_entropy=False, records=False):
    """{item position: frame} from one single-dictionary handle per entry (and one without)."""
    its = record_items() if records else items(max_chunk)
    want = {}
    for e in [-1] + list(range(NENT)):
        pos = [i for i, (_, x) in enumerate(its) if x == e]
        if not pos:
            continue
        fr, _, st, _ = compress([its[i][0] for i in pos], level, max_chunk, dictionary=None if e < 0 else entries()[e], checksum=checksum,
                                dict_entropy=dict_entropy)
        assert st == [0] * len(pos)
        want.update(zip(pos, fr))
    return want


def frame_dict_id(frame):
    """Dictionary_ID of a frame header (0: none)."""
    fhd = frame[4]
    n = (0, 1, 2, 4)[fhd & 3]
    at = 5 + (0 if fhd & 0x20 else 1)
    return int.from_bytes(frame[at:at + n], "little") if n else 0


@functools.lru_cache(maxsize=None)
def table_entries():
    """entries() and six more raw ones, so that content lengths 511, 512, 513, 65,535, 65,536, 65,537
    and 131,072, a formatted dictionary, a constant byte and a period-3 pattern are all in one set."""
    rng = np.random.default_rng(0x5EED0D30)
    out = entries() + [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (513, 65535, 65536, 65537)]
    out += [bytes([0x41]) * 4099, bytes([1, 2, 3]) * 1667]
    assert all(T.dict_layout(e)[0] == 0 for e in out[NENT:])
    return out


def test_tables_equal_host_model(libzstd):
    """Every dictionary's K1 tables, deep-matcher links [0, split), head table, P, dP and split equal
    the host model (zh_dict_tables_model.py) exactly: through entry k of a set (zh_test_dictset_tables)
    and through a handle's load of the same bytes (zh_test_dict_tables, a set of one), which alone
    takes dictionaries under 256 bytes."""
    import cuda_zstd
    import zh_dict_tables_model as M

    L = cuda_zstd.lib()
    vp, u32p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)
    L.zh_test_dictset_tables.restype = ctypes.c_int
    L.zh_test_dictset_tables.argtypes = [vp, ctypes.c_size_t, vp, u32p, vp, vp, u32p, u32p]
    L.zh_test_dict_tables.restype = ctypes.c_int
    L.zh_test_dict_tables.argtypes = [vp, ctypes.c_size_t, vp, u32p, vp, vp, u32p, u32p]

    def tables(call, *first):
        dtab, prev, head = np.full(1 << 15, 0xBEEF, np.uint16), np.full(65536, 0xDEADBEEF, np.uint32), np.full(1 << 14, 0xDEADBEEF, np.uint32)
        P, dP, split = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        assert call(*first, dtab.ctypes.data, ctypes.byref(P), prev.ctypes.data, head.ctypes.data, ctypes.byref(dP), ctypes.byref(split)) == 0
        return dtab, prev, head, P.value, dP.value, split.value

    def check(got, e, tag):
        dtab, prev, head, P, dP, split = got
        content = np.frombuffer(e, np.uint8)[T.dict_layout(e)[1]:]
        cn = len(content)
        wP, wtab = M.k1_tables(content)
        wdP, wsplit, wprev, whead = M.deep_chains(content)
        assert (P, dP, split) == (wP, wdP, wsplit), (tag, P, dP, split)
        assert P == (0 if cn < 512 else min(cn, 65535)) and (dP, split) == ((0, 0) if cn < 72 else (min(cn, 65536), (min(cn, 65536) - 8) & ~3)), tag
        if P:
            assert np.array_equal(dtab, wtab), tag
        else:  # untouched
            assert bool((dtab == 0xBEEF).all()), tag
        if dP:
            assert np.array_equal(prev[:split], wprev) and np.array_equal(head, whead), tag
        else:
            assert bool((head == 0xDEADBEEF).all()), tag
        assert bool((prev[split:] == 0xDEADBEEF).all()), tag
        return P, dP

    ents = table_entries()
    s = cuda_zstd.DictionarySet([cuda_zstd.Dictionary.load(e) for e in ents])
    assert len(s) == len(ents) == NENT + 6
    seen = []
    for k, e in enumerate(ents):
        buf = np.frombuffer(e, np.uint8).copy()
        seen.append(check(tables(L.zh_test_dictset_tables, s._h, k), e, ("set", k)))
        assert check(tables(L.zh_test_dict_tables, buf.ctypes.data, len(buf)), e, ("load", k)) == seen[-1]
    s.close()
    assert seen[0][0] == 0 and seen[1][0] == 0 and seen[2][0] == 512 and seen[5] == (65535, 65536)
    assert seen[NENT:] == [(513, 513), (65535, 65535), (65535, 65536), (65535, 65536), (4099, 4099), (5001, 5001)]
    assert 0 < seen[JSON_D][0] < 16384 and 0 < seen[TEXT_D][0] < 16384  # the formatted entries: their content alone
    # a handle's dictionary may be shorter than a set's entries: no chains below 72 bytes
    rng = np.random.default_rng(0x5EED0D31)
    small = {n: rng.integers(0, 256, n, dtype=np.uint8) for n in (1, 71, 72, 75, 255)}
    got = {n: check(tables(L.zh_test_dict_tables, b.ctypes.data, n), b.tobytes(), ("load", n)) for n, b in small.items()}
    assert got == {1: (0, 0), 71: (0, 0), 72: (0, 72), 75: (0, 75), 255: (0, 255)}


@pytest.mark.parametrize("level,max_chunk,checksum", [(1, 65536, False), (3, 65536, False), (3, 32768, False), (3, 65536, True), (5, 65536, False),
                                                       (9, 65536, False)])
def test_compress_equals_single_dictionary_handle(libzstd, level, max_chunk, checksum):
    its = items(max_chunk)
    frames, sizes, st, raw = set_frames(level, max_chunk, checksum)
    want = single_frames(level, max_chunk, checksum)
    ents = entries()
    ids = [T.dict_layout(e)[0] for e in ents]
    bad = [i for i, (_, e) in enumerate(its) if e < -1 or e >= NENT]
    assert bad == [3, 10] and len(want) == len(its) - 2
    used = set()
    for i, ((c, e), f) in enumerate(zip(its, frames)):
        if i in bad:  # size 0, status 2, output slot untouched
            assert st[i] == INVALID and sizes[i] == 0 and bool((raw[i] == SENTINEL).all()), i
            continue
        assert st[i] == 0 and f == want[i], (i, len(c), e)
        assert frame_dict_id(f) == (ids[e] if e >= 0 else 0), (i, e)
        assert T.zstd_decompress(f, len(c), dictionary=ents[e] if e >= 0 else None) == c.tobytes(), (i, e)
        if level == 3 and e in (JSON_D, TEXT_D):
            assert f == T.oracle_frame(c, dictionary=ents[e], level=3, checksum=checksum), (i, e)
        used.add(e)
    assert used == set(range(-1, NENT))


@functools.lru_cache(maxsize=None)
def record_items():
    """64 records of 300 .. 1,024 bytes against the two formatted entries, interleaved, then two
    against a raw entry."""
    rng = np.random.default_rng(0x5EED0D20)
    js = T.gen(T.DG_JSON, 1, 0x5EED0D21, 64 * 1024)
    tx = T.gen(T.DG_TEXT, 1, 0x5EED0D22, 64 * 1024)
    out = []
    for k in range(64):
        n = int(rng.integers(300, 1025))
        out.append(((js if k % 2 == 0 else tx)[k * 1024:k * 1024 + n], JSON_D if k % 2 == 0 else TEXT_D))
    out += [(js[:700], 2), (tx[:900], 5)]
    return out


def test_dict_entropy(libzstd):
    its = record_items()
    chunks, idx = [c for c, _ in its], [e for _, e in its]
    on, son, st, _ = compress(chunks, 3, 1024, idx=idx, dict_entropy=True)
    off, soff, st2, _ = compress(chunks, 3, 1024, idx=idx)
    assert st == [0] * len(its) == st2
    want = single_frames(3, 1024, dict_entropy=True, records=True)
    ents = entries()
    for i, ((c, e), f) in enumerate(zip(its, on)):
        assert f == want[i], (i, e)
        assert T.zstd_decompress(f, len(c), dictionary=ents[e]) == c.tobytes(), i
    assert sum(son) < sum(soff), (sum(son), sum(soff))
    assert on[64:] == off[64:]  # a raw entry has no entropy section: the switch changes nothing


def zstd_dict_nofcs(data, dictionary, level):
    """libzstd frame with the dictionary loaded and no Frame_Content_Size (ZSTD_CCtx_loadDictionary +
    ZSTD_compress2 with contentSizeFlag, 200, off)."""
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


@functools.lru_cache(maxsize=None)
def id_batch():
    """[(frame, decoded bytes)] whose dictionaries the decoder finds by Dictionary_ID: libzstd frames
    of records of 300 B .. 200 KiB against the two formatted entries (levels 1, 3, 19; with and
    without a content size), this library's set-compressed frames of those entries, plain frames."""
    ents = entries()
    out = []
    for e, kind in ((JSON_D, T.DG_JSON), (TEXT_D, T.DG_TEXT)):
        d = ents[e]
        for j, n in enumerate((300, 1000, 40000)):
            rec = stream_of(kind, 200 + 10 * e + j, n)
            for level in (1, 3, 19):
                out.append((T.zstd_compress_dict(rec, d, level), rec.tobytes()))
        big = stream_of(kind, 260 + e, 200000)
        out.append((T.zstd_compress_dict(big, d, 3), big.tobytes()))
        for j, n in enumerate((300, 700, 200000)):
            rec = stream_of(kind, 270 + 10 * e + j, n)
            out.append((zstd_dict_nofcs(rec, d, 3), rec.tobytes()))
    for f, _ in out:
        assert frame_dict_id(f) in (T.dict_layout(ents[JSON_D])[0], T.dict_layout(ents[TEXT_D])[0])
    its = items(65536)
    frames = set_frames(3, 65536)[0]
    own = [(frames[i], c.tobytes()) for i, (c, e) in enumerate(its) if e in (-1, JSON_D, TEXT_D)]
    assert len(own) >= 12
    out += own
    for f, want in out:  # the reference: libzstd with the right dictionary
        did = frame_dict_id(f)
        d = None if not did else ents[JSON_D] if did == T.dict_layout(ents[JSON_D])[0] else ents[TEXT_D]
        assert T.zstd_decompress(f, len(want), dictionary=d) == want
    return out


def patched_id(frame):
    """The frame with its Dictionary_ID changed to one the set does not hold."""
    b = bytearray(frame)
    assert b[4] & 3
    at = 5 + (0 if b[4] & 0x20 else 1)
    b[at] ^= 0x55
    assert frame_dict_id(bytes(b)) not in [0] + [T.dict_layout(e)[0] for e in entries()]
    return bytes(b)


def decode(frames, caps, idx=None, total=None, sizes_only=False):
    """frames (cycled to `total` buffers) through the bound set -> (out, offsets, sizes, statuses);
    idx None: a null index array.  sizes_only: the size query instead."""
    import torch

    import cuda_zstd

    m = len(frames)
    n = total or m
    fa = Arena(frames)
    sel = [i % m for i in range(n)]
    max_out = max(max(caps), 1)
    offs = np.concatenate([[0], np.cumsum([caps[k] + 3 for k in sel])])
    out = torch.full((int(offs[-1]) + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    bd = cuda_zstd.BatchedDecompressor()
    bd.set_dictionary_set(dset())
    out_sizes = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    in_ptrs, in_sizes = i64(fa.ptrs[k] for k in sel), i64(fa.sizes[k] for k in sel)
    if sizes_only:
        bd.get_sizes_async(in_ptrs, in_sizes, out_sizes, status)
    else:
        temp = torch.empty(bd.temp_size(n, max_out), dtype=torch.uint8, device="cuda")
        args = (i64(caps[k] for k in sel), max_out, i64(out.data_ptr() + int(offs[i]) for i in range(n)), out_sizes, status, temp)
        if idx is None and total is None:
            bd.decompress_async(in_ptrs, in_sizes, *args)  # the plain entry resolves by ID too
        else:
            bd.decompress_dicts_async(in_ptrs, in_sizes, None if idx is None else i32(idx[k] for k in sel), *args)
    torch.cuda.synchronize()
    bd.close()
    return out, offs, out_sizes.cpu().tolist(), status.cpu().tolist()


@functools.lru_cache(maxsize=None)
def decode_cases():
    """id_batch plus the cases of the issue -> (frames, expected bytes or None, indices, expected status)."""
    ents = entries()
    base = id_batch()
    frames, wants = [f for f, _ in base], [w for _, w in base]
    idx, st = [-1] * len(base), [0] * len(base)
    first_js = next(i for i, (f, _) in enumerate(base) if frame_dict_id(f) == T.dict_layout(ents[JSON_D])[0])
    first_tx = next(i for i, (f, _) in enumerate(base) if frame_dict_id(f) == T.dict_layout(ents[TEXT_D])[0])

    def add(f, w, e, s):
        frames.append(f), wants.append(w), idx.append(e), st.append(s)

    # an ID the set does not hold, between good neighbours
    add(patched_id(base[first_js][0]), None, -1, DICT_WRONG)
    # two frames naming the two formatted entries in one buffer
    add(base[first_js][0] + base[first_tx][0], base[first_js][1] + base[first_tx][1], -1, 0)
    add(base[first_tx][0], base[first_tx][1], -1, 0)
    n_id = len(frames)  # everything up to here needs no index
    # a raw-content entry's frame: by index it decodes, by ID (-1) it cannot
    # (a record that repeats 2,000 bytes of the entry's tail, so the frame does reach into it)
    rec = np.concatenate([np.frombuffer(ents[5], np.uint8)[-3000:-1000], stream_of(T.DG_JSON, 300, 500)])
    (raw_f,), _, raw_st, _ = compress([rec], 3, 65536, idx=[5])
    assert raw_st == [0] and frame_dict_id(raw_f) == 0 and len(raw_f) < 1000
    assert T.zstd_decompress(raw_f, len(rec), dictionary=ents[5]) == rec.tobytes()
    with pytest.raises(AssertionError):
        T.zstd_decompress(raw_f, len(rec))
    add(raw_f, rec.tobytes(), 5, 0)
    add(raw_f, rec.tobytes(), -1, "not ok with the right bytes")
    # a formatted frame with the other formatted entry's index; its own index; an index past the set
    add(base[first_js][0], None, TEXT_D, DICT_WRONG)
    add(base[first_js][0], base[first_js][1], JSON_D, 0)
    add(base[first_js][0], None, NENT, INVALID)
    add(base[first_tx][0], base[first_tx][1], -1, 0)
    return frames, wants, idx, st, n_id


def check_outputs(out, offs, sizes, got_st, wants, st, sel):
    host = out.cpu().numpy()
    for i, k in enumerate(sel):
        at = int(offs[i])
        if st[k] == 0:
            assert got_st[i] == 0 and sizes[i] == len(wants[k]) and host[at:at + sizes[i]].tobytes() == wants[k], (i, k)
        elif isinstance(st[k], str):
            assert not (got_st[i] == 0 and host[at:at + len(wants[k])].tobytes() == wants[k]), (i, k)
        else:
            assert got_st[i] == st[k] and sizes[i] == 0, (i, k, got_st[i])


def test_decode_resolves_dictionaries(libzstd):
    frames, wants, idx, st, n_id = decode_cases()
    caps = [len(w) if w is not None else 70000 for w in wants]
    # a null index array (the plain entry): everything that needs no index
    out, offs, sizes, got = decode(frames[:n_id], caps[:n_id])
    check_outputs(out, offs, sizes, got, wants, st, range(n_id))
    # the same call with indices: -1 resolves by ID, >= 0 names the entry
    out, offs, sizes, got = decode(frames, caps, idx=idx)
    check_outputs(out, offs, sizes, got, wants, st, range(len(frames)))


def test_decode_split_pipeline(libzstd):
    """300 copies of the ID-resolved batch: the deferred (tables / rest / sequence / execution)
    kernels and the walker all resolve dictionaries."""
    frames, wants, idx, st, n_id = decode_cases()
    caps = [len(w) if w is not None else 70000 for w in wants]
    assert n_id >= 30 and any(s == DICT_WRONG for s in st[:n_id])
    total = 300 * n_id
    assert total >= 2048
    out, offs, sizes, got = decode(frames[:n_id], caps[:n_id], total=total)
    check_outputs(out, offs, sizes, got, wants, st, [i % n_id for i in range(total)])


def test_size_query(libzstd):
    frames, wants, idx, st, n_id = decode_cases()
    caps = [len(w) if w is not None else 70000 for w in wants]
    _, _, sizes, got = decode(frames[:n_id], caps[:n_id], sizes_only=True)
    nofcs = 0
    for k in range(n_id):
        if st[k] == 0:
            assert got[k] == 0 and sizes[k] == len(wants[k]), k
            nofcs += (frames[k][4] >> 6) == 0 and not (frames[k][4] & 0x20)
        else:
            assert got[k] == DICT_WRONG and sizes[k] == 0, k
    assert nofcs >= 6  # frames without a content size, small ones' first blocks on dictionary tables


def test_unbound_and_exclusive(libzstd):
    import torch

    import cuda_zstd

    its = [x for x in items(65536) if 0 <= x[1] < NENT][:6]
    n, cs = len(its), 65536
    ar = Arena([c for c, _ in its])
    bc = cuda_zstd.BatchedCompressor(3)
    slot = (bc.max_out(cs) + 255) // 256 * 256
    out = torch.full((n * slot,), SENTINEL, dtype=torch.uint8, device="cuda")
    optr = i64(out.data_ptr() + i * slot for i in range(n))
    osz = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    args = (i64(ar.ptrs), i64(ar.sizes), i32(e for _, e in its))
    full = torch.empty(bc.temp_size_dicts(n, cs), dtype=torch.uint8, device="cuda")
    with pytest.raises(cuda_zstd.ZstdError) as e:  # no set bound
        bc.compress_dicts_async(*args, cs, optr, osz, st, full)
    assert e.value.code == 2
    bc.set_dictionary_set(dset())
    with pytest.raises(cuda_zstd.ZstdError) as e:  # a workspace one byte short
        bc.compress_dicts_async(*args, cs, optr, osz, st, full[:-1])
    assert e.value.code == 7
    with pytest.raises(cuda_zstd.ZstdError) as e:  # a null index array
        bc.compress_dicts_async(args[0], args[1], None, cs, optr, osz, st, full)
    assert e.value.code == 2
    one = cuda_zstd.Dictionary.load(entries()[JSON_D])
    with pytest.raises(cuda_zstd.ZstdError) as e:  # a dictionary while a set is bound
        bc.set_dictionary(one)
    assert e.value.code == 2
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((osz == -7).all()) and bool((st == -1).all())  # nothing was launched
    bc.set_dictionary_set(None)
    bc.set_dictionary(one)
    with pytest.raises(cuda_zstd.ZstdError) as e:  # a set while a dictionary is set
        bc.set_dictionary_set(dset())
    assert e.value.code == 2
    bc.close()
    bd = cuda_zstd.BatchedDecompressor()
    dtemp = torch.empty(bd.temp_size(n, cs), dtype=torch.uint8, device="cuda")
    with pytest.raises(cuda_zstd.ZstdError) as e:  # the decode entry without a set
        bd.decompress_dicts_async(args[0], args[1], None, None, cs, optr, osz, st, dtemp)
    assert e.value.code == 2
    bd.close()
    assert len(dset()) == NENT and cuda_zstd.lib().cuda_zstd_dict_set_count(None) == 0


def test_two_streams_and_destroy(libzstd):
    """Two streams compress with one set at the same time; the set is destroyed right after the
    calls were issued (destroy waits for their events) and the frames are right."""
    import torch

    import cuda_zstd

    its = [x for x in items(65536) if -1 <= x[1] < NENT]
    chunks, idx = [c for c, _ in its], [e for _, e in its]
    n, cs = len(its), 65536
    ar = Arena(chunks)
    s = cuda_zstd.DictionarySet([cuda_zstd.Dictionary.load(e) for e in entries()])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    runs = []
    for sm in streams:
        bc = cuda_zstd.BatchedCompressor(3)
        bc.set_dictionary_set(s)
        slot = (bc.max_out(cs) + 255) // 256 * 256
        with torch.cuda.stream(sm):
            out = torch.full((n * slot,), SENTINEL, dtype=torch.uint8, device="cuda")
            osz = torch.full((n,), -7, dtype=torch.int64, device="cuda")
            st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            temp = torch.empty(bc.temp_size_dicts(n, cs), dtype=torch.uint8, device="cuda")
            tabs = (i64(ar.ptrs), i64(ar.sizes), i32(idx), i64(out.data_ptr() + i * slot for i in range(n)))
            bc.compress_dicts_async(tabs[0], tabs[1], tabs[2], cs, tabs[3], osz, st, temp, sm)
        runs.append((bc, out, osz, st, temp, tabs, slot))
    for r in runs:
        r[0].close()  # (the handles let go of the set)
    s.close()
    torch.cuda.synchronize()
    want = single_frames(3, 65536)
    pos = [i for i, (_, e) in enumerate(items(65536)) if -1 <= e < NENT]
    for _, out, osz, st, _, _, slot in runs:
        sizes, host = osz.cpu().tolist(), out.cpu().numpy()
        assert st.cpu().tolist() == [0] * n
        assert [host[i * slot:i * slot + sizes[i]].tobytes() for i in range(n)] == [want[p] for p in pos]

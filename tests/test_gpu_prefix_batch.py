"""Batched compression and decompression with one prefix per chunk
(nvcomp_zstd_batched_compress_prefix_async_v5 / nvcomp_zstd_batched_decompress_prefix_async_v5;
the per-item prefix of csrc/zh_block_plan.h, zh_plan_kernel and the decoder's item_view).

The items come from the grid sizes x prefix lengths of the issue; chunk and prefix are cut from one
stream of JSON or text and sit at odd addresses of one device arena.  The oracle's frames and the GPU
frames of a (level, max_chunk) batch are computed once per module and shared read-only."""
import ctypes
import functools

import numpy as np
import pytest

import zh_testlib as T

pytestmark = pytest.mark.gpu

SIZES = [1, 32767, 32768, 32769, 65536, 65537, 163840]
PREFIXES = [0, 1, 32767, 32768, 65535, 65536]
SENTINEL = 0xA5
CORRUPT, DICT_WRONG = 6, 1  # nvcomp-style codes of the decoder (zh_decode.hip to_nvcomp)


@functools.lru_cache(maxsize=None)
def stream_of(k, total):
    return T.gen(T.DG_JSON if k % 2 == 0 else T.DG_TEXT, 1, 0x5EED0C00 + k, total)


@functools.lru_cache(maxsize=None)
def items(max_chunk):
    """[(chunk, prefix or None)]: every grid size up to max_chunk x every prefix length, then one
    chunk behind a 200,000-byte prefix and the same chunk behind that prefix's last 65,536 bytes."""
    out = []
    for n in SIZES:
        if n > max_chunk:
            continue
        for pn in PREFIXES:
            s = stream_of(len(out), pn + n)
            out.append((s[pn:], s[:pn] if pn else None))
    s = stream_of(1000, 200000 + 40000)
    out.append((s[200000:], s[:200000]))
    out.append((s[200000:], s[200000 - 65536:200000]))
    return out


@functools.lru_cache(maxsize=None)
def oracle(level, max_chunk):
    return [T.oracle_frame(c, dictionary=(p[-65536:].tobytes() if p is not None else None), level=level) for c, p in items(max_chunk)]


class Arena:
    """Host buffers laid out at odd addresses of one device allocation (None: pointer 0, size 0)."""

    def __init__(self, bufs):
        import torch

        self.off, o = [], 1
        for b in bufs:
            self.off.append(o)
            o += (len(b) if b is not None else 0) + 2
            o |= 1
        host = np.zeros(o + 256, np.uint8)
        for b, at in zip(bufs, self.off):
            if b is not None and len(b):
                host[at:at + len(b)] = np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else b
        self.dev = torch.from_numpy(host).cuda()
        base = self.dev.data_ptr()
        assert base % 16 == 0
        self.ptrs = [base + at if b is not None and len(b) else 0 for b, at in zip(bufs, self.off)]
        self.sizes = [len(b) if b is not None else 0 for b in bufs]
        assert all(p % 2 == 1 for p in self.ptrs if p)


def i64(v):
    import torch

    return torch.tensor(list(v), dtype=torch.int64, device="cuda")


def compress(pairs, level, max_chunk, prefix_ptr_override=None, plain=False, checksum=False):
    """One call over (chunk, prefix) pairs -> (frames, sizes, statuses, raw outputs)."""
    import torch

    import cuda_zstd

    n = len(pairs)
    chunks, pres = Arena([c for c, _ in pairs]), Arena([p for _, p in pairs])
    bc = cuda_zstd.BatchedCompressor(level, 65536, checksum=checksum)
    slot = (bc.max_out(max_chunk) + 255) // 256 * 256
    out = torch.full((n * slot,), SENTINEL, dtype=torch.uint8, device="cuda")
    pre_ptrs, pre_sizes = list(pres.ptrs), list(pres.sizes)
    for k, (ptr, size) in (prefix_ptr_override or {}).items():
        pre_ptrs[k], pre_sizes[k] = ptr, size
    out_ptrs = i64(out.data_ptr() + i * slot for i in range(n))
    out_sizes = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    if plain:
        temp = torch.empty(bc.temp_size(n, max_chunk), dtype=torch.uint8, device="cuda")
        bc.compress_async(i64(chunks.ptrs), i64(chunks.sizes), max_chunk, out_ptrs, out_sizes, status, temp)
    else:
        temp = torch.empty(bc.temp_size_prefix(n, max_chunk), dtype=torch.uint8, device="cuda")
        bc.compress_prefix_async(i64(chunks.ptrs), i64(chunks.sizes), i64(pre_ptrs), i64(pre_sizes), max_chunk, out_ptrs, out_sizes, status, temp)
    torch.cuda.synchronize()
    bc.close()
    sizes, st, host = out_sizes.cpu().tolist(), status.cpu().tolist(), out.cpu().numpy()
    frames = [host[i * slot:i * slot + max(sizes[i], 0)].tobytes() for i in range(n)]
    return frames, sizes, st, [host[i * slot:(i + 1) * slot] for i in range(n)]


@functools.lru_cache(maxsize=None)
def gpu_frames(level, max_chunk):
    """The batch of items(max_chunk) plus, last, one item with a null prefix pointer and size 100."""
    pairs = list(items(max_chunk)) + [(stream_of(2000, 5000), None)]
    return compress(pairs, level, max_chunk, prefix_ptr_override={len(pairs) - 1: (0, 100)})


def decompress(frames, prefixes, caps, total=None):
    """frames[i] behind prefixes[i] (cycled to `total` buffers) -> (outputs, sizes, statuses)."""
    import torch

    import cuda_zstd

    m = len(frames)
    n = total or m
    fa, pa = Arena(frames), Arena(prefixes)
    max_out = max(max(caps), 1)
    offs = np.concatenate([[0], np.cumsum([caps[i % m] + 3 for i in range(n)])])
    out = torch.full((int(offs[-1]) + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    idx = [i % m for i in range(n)]
    bd = cuda_zstd.BatchedDecompressor()
    temp = torch.empty(bd.temp_size(n, max_out), dtype=torch.uint8, device="cuda")
    out_sizes = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    bd.decompress_prefix_async(i64(fa.ptrs[k] for k in idx), i64(fa.sizes[k] for k in idx), i64(pa.ptrs[k] for k in idx),
                               i64(pa.sizes[k] for k in idx), i64(caps[k] for k in idx), max_out,
                               i64(out.data_ptr() + int(offs[i]) for i in range(n)), out_sizes, status, temp)
    torch.cuda.synchronize()
    bd.close()
    return out, offs, out_sizes.cpu().tolist(), status.cpu().tolist()


def check_decode(frames, prefixes, datas, total=None):
    """Every buffer decodes byte-exact with status 0 (compared on the device in one piece)."""
    import torch

    m = len(frames)
    out, offs, sizes, st = decompress(frames, prefixes, [len(d) for d in datas], total)
    n = len(sizes)
    assert st == [0] * n
    assert sizes == [len(datas[i % m]) for i in range(n)]
    want = np.full(int(offs[-1]) + 16, SENTINEL, np.uint8)
    for i in range(n):
        d = datas[i % m]
        want[int(offs[i]):int(offs[i]) + len(d)] = np.frombuffer(bytes(d), np.uint8) if not isinstance(d, np.ndarray) else d
    assert torch.equal(out, torch.from_numpy(want).cuda())


@pytest.mark.parametrize("max_chunk", [65536, 163840])
@pytest.mark.parametrize("level", [1, 3, 9])
def test_compress_parity(libzstd, level, max_chunk):
    pairs = items(max_chunk)
    frames, sizes, st, raw = gpu_frames(level, max_chunk)
    want = oracle(level, max_chunk)
    n = len(pairs)
    assert 30 <= n <= 46
    assert st[:n] == [0] * n and sizes[:n] == [len(w) for w in want]
    for i, ((c, p), f, w) in enumerate(zip(pairs, frames, want)):
        assert f == w, (i, len(c), None if p is None else len(p))
        assert T.zstd_decompress(f, len(c), dictionary=None if p is None else p.tobytes()) == c.tobytes(), i
    # a prefix of 200,000 bytes: the frame of its last 65,536 bytes (decoded above with the whole prefix)
    assert len(pairs[n - 2][1]) == 200000 and frames[n - 2] == frames[n - 1]
    # items without a prefix: the plain entry's frames of the same chunks
    bare = [i for i, (_, p) in enumerate(pairs) if p is None]
    assert len(bare) == len([s for s in SIZES if s <= max_chunk])
    pf, _, pst, _ = compress([(pairs[i][0], None) for i in bare], level, max_chunk, plain=True)
    assert pst == [0] * len(bare) and pf == [frames[i] for i in bare]
    # a null prefix pointer with a non-zero size: status 2, size 0, output untouched
    assert st[n] == 2 and sizes[n] == 0 and bool((raw[n] == SENTINEL).all())


def test_refusals(libzstd):
    import torch

    import cuda_zstd

    pairs = items(65536)[:6]
    n, cs = len(pairs), 65536
    chunks, pres = Arena([c for c, _ in pairs]), Arena([p for _, p in pairs])
    bc = cuda_zstd.BatchedCompressor(3)
    slot = (bc.max_out(cs) + 255) // 256 * 256
    out = torch.full((n * slot,), SENTINEL, dtype=torch.uint8, device="cuda")
    optr = i64(out.data_ptr() + i * slot for i in range(n))
    osz = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    args = (i64(chunks.ptrs), i64(chunks.sizes), i64(pres.ptrs), i64(pres.sizes))
    short = torch.empty(bc.temp_size_prefix(n, cs) - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(cuda_zstd.ZstdError) as e:  # a workspace one byte short
        bc.compress_prefix_async(*args, cs, optr, osz, st, short)
    assert e.value.code == 7
    full = torch.empty(bc.temp_size_prefix(n, cs), dtype=torch.uint8, device="cuda")
    with pytest.raises(cuda_zstd.ZstdError) as e:  # a null prefix array
        bc.compress_prefix_async(args[0], args[1], None, args[3], cs, optr, osz, st, full)
    assert e.value.code == 2
    with pytest.raises(cuda_zstd.ZstdError) as e:  # max_chunk == 0
        bc.compress_prefix_async(*args, 0, optr, osz, st, full)
    assert e.value.code == 2
    L = cuda_zstd.lib()
    assert L.nvcomp_zstd_batched_compress_prefix_async_v5(bc._h, None, None, None, None, cs, 0, None, None, None, None, 0, None) == 0
    bc.set_dictionary(cuda_zstd.Dictionary.load(T.gen(T.DG_JSON, 1, 0x5EED0C06, 16384).tobytes()))
    with pytest.raises(cuda_zstd.ZstdError) as e:  # a handle with a dictionary
        bc.compress_prefix_async(*args, cs, optr, osz, st, full)
    assert e.value.code == 2
    dtemp = torch.empty(cuda_zstd.BatchedDecompressor.temp_size(n, cs), dtype=torch.uint8, device="cuda")
    rc = L.nvcomp_zstd_batched_decompress_prefix_async_v5(bc._h, args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), args[3].data_ptr(),
                                                          None, cs, n, optr.data_ptr(), osz.data_ptr(), st.data_ptr(), dtemp.data_ptr(),
                                                          dtemp.numel(), None)
    assert rc == 2
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((osz == -7).all()) and bool((st == -1).all())
    bc.close()


def test_delta(libzstd):
    """32 chunks of 32 KiB, each its 32 KiB prefix with 16 bytes changed: the prefix pays."""
    rng = np.random.default_rng(0x5EED0C01)
    base = T.gen(T.DG_JSON, 32, 0x5EED0C02, 32768)
    pairs = []
    for i in range(32):
        p = base[i * 32768:(i + 1) * 32768]
        c = p.copy()
        at = int(rng.integers(0, 32768 - 16))
        c[at:at + 16] = rng.integers(0, 256, 16, dtype=np.uint8)
        pairs.append((c, p))
    frames, sizes, st, _ = compress(pairs, 3, 32768)
    bare, bsizes, bst, _ = compress([(c, None) for c, _ in pairs], 3, 32768)
    assert st == [0] * 32 == bst
    tot_h, tot_p = sum(sizes), sum(bsizes)
    assert tot_h < tot_p, (tot_h, tot_p)
    for i, ((c, p), f) in enumerate(zip(pairs, frames)):
        assert f == T.oracle_frame(c, dictionary=p.tobytes(), level=3), i
    assert bare == [T.oracle_frame(c, level=3) for c, _ in pairs]


@pytest.mark.parametrize("total", [None, 2304], ids=["one_stream", "split_pipeline"])
@pytest.mark.parametrize("max_chunk", [65536, 163840])
def test_decode_own_frames(libzstd, max_chunk, total):
    pairs = items(max_chunk)
    frames = gpu_frames(3, max_chunk)[0][:len(pairs)]
    check_decode(frames, [p for _, p in pairs], [c for c, _ in pairs], total)


@functools.lru_cache(maxsize=None)
def far_inputs():
    """A 200,000-byte prefix and chunks of 60,000 and 300,000 bytes that repeat material from the
    prefix's first 4 KiB (offsets past 128 KiB) -> (prefix, [(chunk, libzstd frame)])."""
    prefix = T.gen(T.DG_TEXT, 1, 0x5EED0C03, 200000)
    rng = np.random.default_rng(0x5EED0C04)
    out = []
    for n in (60000, 300000):
        fresh = T.gen(T.DG_JSON, 1, 0x5EED0C05 + n, n)
        c = fresh.copy()
        at = 0
        while at + 600 < n:
            src = int(rng.integers(0, 4096 - 300))
            c[at:at + 300] = prefix[src:src + 300]
            at += 3000
        for level in (1, 3, 19):
            out.append((c, T.zstd_compress_dict(c, prefix.tobytes(), level)))
    return prefix, out


@pytest.mark.parametrize("total", [None, 2304], ids=["one_stream", "split_pipeline"])
def test_decode_libzstd_frames(libzstd, total):
    prefix, fr = far_inputs()
    reach = []
    for c, f in fr:  # on the CPU first: the whole prefix decodes, and (some level) the last 128 KiB alone does not
        assert T.zstd_decompress(f, len(c), dictionary=prefix.tobytes()) == c.tobytes()
        try:
            reach.append(T.zstd_decompress(f, len(c), dictionary=prefix[-131072:].tobytes()) != c.tobytes())
        except AssertionError:
            reach.append(True)
    assert any(reach)
    check_decode([f for _, f in fr], [prefix] * len(fr), [c for c, _ in fr], total)


def test_rejects(libzstd):
    rng = np.random.default_rng(0x5EED0C07)
    prefix = rng.integers(0, 256, 4096, dtype=np.uint8)
    chunk = np.concatenate([prefix[:2000], rng.integers(0, 256, 500, dtype=np.uint8)])
    frame = T.zstd_compress_dict(chunk, prefix.tobytes(), 3)
    assert len(frame) < 1500 and T.zstd_decompress(frame, len(chunk), dictionary=prefix.tobytes()) == chunk.tobytes()
    for d in (prefix[-1024:].tobytes(), None):  # libzstd rejects both
        with pytest.raises(AssertionError):
            T.zstd_decompress(frame, len(chunk), dictionary=d)
    # a frame that names Dictionary_ID 7: magic, FHD (single segment, 1-byte ID), ID, FCS 3, one raw last block
    with_id = bytes([0x28, 0xB5, 0x2F, 0xFD, 0x21, 7, 3, 0x19, 0, 0]) + b"abc"
    with pytest.raises(AssertionError, match="[Dd]ictionary"):
        T.zstd_decompress(with_id, 3)
    good = T.oracle_frame(chunk, level=3)
    frames = [good, frame, frame, good, with_id, frame, good]
    pres = [None, prefix[-1024:], None, prefix, prefix, prefix, None]
    out, offs, sizes, st = decompress(frames, pres, [len(chunk)] * len(frames))
    assert st == [0, CORRUPT, CORRUPT, 0, DICT_WRONG, 0, 0]
    host = out.cpu().numpy()
    for i, s in enumerate(st):
        if s == 0:
            assert sizes[i] == len(chunk) and host[int(offs[i]):int(offs[i]) + len(chunk)].tobytes() == chunk.tobytes(), i
        else:
            assert sizes[i] == 0, i


def test_python_surface(libzstd):
    import torch

    import cuda_zstd

    pairs = items(65536)[:14]
    want = oracle(3, 65536)[:14]
    chunks = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c, _ in pairs]
    pres = [None if p is None else torch.from_numpy(np.ascontiguousarray(p)).cuda() for _, p in pairs]
    frames = cuda_zstd.compress_batch_prefix(chunks, pres, level=3)
    assert [f.cpu().numpy().tobytes() for f in frames] == want
    back = cuda_zstd.decompress_batch_prefix(frames, pres)
    assert [b.cpu().numpy().tobytes() for b in back] == [c.tobytes() for c, _ in pairs]
    hf = cuda_zstd.compress_batch_prefix([c.tobytes() for c, _ in pairs], [None if p is None else p.tobytes() for _, p in pairs])
    assert hf == want
    assert cuda_zstd.decompress_batch_prefix(hf, [None if p is None else p for _, p in pairs]) == [c.tobytes() for c, _ in pairs]
    assert cuda_zstd.compress_batch_prefix([], []) == [] and cuda_zstd.decompress_batch_prefix([], []) == []

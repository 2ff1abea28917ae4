"""Batched compression at one level per chunk, read on the device
(nvcomp_zstd_batched_compress_levels_async_v5; zh_rank_kernel, zh_plan_levels_kernel and the ranged
matcher launches of csrc/zh_plan.hip, zh_lz.hip, zh_lz_deep.hip).

A frame is "compared as described" when it equals the oracle's frame at its level
(T.oracle_frame(chunk, level=lv)), equals the frame a single-level handle writes for the chunk
through nvcomp_zstd_batched_compress_async_v5 with the same max_uncompressed_chunk_bytes, and
decodes with libzstd.  The oracle's frames of the shared batch are computed once per module."""
import functools

import numpy as np
import pytest

import zh_testlib as T

pytestmark = pytest.mark.gpu

SELECTOR_LEVELS = [1, 3, 5, 6, 9, 12, 16, 19]  # zh_adaptive_level's table
CYCLE = [1, 2, 3, 4, 5, 6, 7, 9, 10, 12, 19, 22]
SENTINEL = 0xA5


def parse_class(level):
    """ZH_LEVEL_CLASS (include/zstd_hip_params.h): K1 mode 2, 1, 0, then the deep depths 128 .. 4."""
    if level <= 4:
        return 0 if level <= 1 else 1 if level == 2 else 2
    depth = 4 if level <= 5 else 8 if level == 6 else 16 if level == 7 else 32 if level <= 9 else 64 if level == 10 else 128
    return {128: 3, 64: 4, 32: 5, 16: 6, 8: 7, 4: 8}[depth]


def run(datas, levels=None, level=3, max_chunk=None, checksum=False):
    """One call over caller-owned device buffers pre-filled with sentinels.  levels: the per-chunk
    entry; none: the existing single-level entry on a handle at `level`.  Returns
    (frames, sizes, statuses, raw outputs) after one synchronise."""
    import torch

    import cuda_zstd

    n = len(datas)
    max_chunk = max_chunk or max(max(len(d) for d in datas), 1)
    bc = cuda_zstd.BatchedCompressor(level, 65536, checksum=checksum)
    slot = (bc.max_out(max_chunk) + 255) // 256 * 256
    ins = [torch.from_numpy(np.ascontiguousarray(d)).cuda() if len(d) else torch.zeros(1, dtype=torch.uint8, device="cuda") for d in datas]
    out = torch.full((n * slot,), SENTINEL, dtype=torch.uint8, device="cuda")
    in_ptrs = torch.tensor([t.data_ptr() for t in ins], dtype=torch.int64, device="cuda")
    in_sizes = torch.tensor([len(d) for d in datas], dtype=torch.int64, device="cuda")
    out_ptrs = torch.tensor([out.data_ptr() + i * slot for i in range(n)], dtype=torch.int64, device="cuda")
    out_sizes = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    if levels is not None:
        d_levels = torch.tensor(list(levels), dtype=torch.int32, device="cuda")
        temp = torch.empty(bc.temp_size_levels(n, max_chunk), dtype=torch.uint8, device="cuda")
        bc.compress_levels_async(in_ptrs, in_sizes, d_levels, max_chunk, out_ptrs, out_sizes, status, temp)
    else:
        temp = torch.empty(bc.temp_size(n, max_chunk), dtype=torch.uint8, device="cuda")
        bc.compress_async(in_ptrs, in_sizes, max_chunk, out_ptrs, out_sizes, status, temp)
    torch.cuda.synchronize()
    bc.close()
    sizes, st, host = out_sizes.cpu().tolist(), status.cpu().tolist(), out.cpu().numpy()
    frames = [host[i * slot:i * slot + max(sizes[i], 0)].tobytes() for i in range(n)]
    return frames, sizes, st, [host[i * slot:(i + 1) * slot] for i in range(n)]


def single_level_frames(datas, levels, max_chunk=None, checksum=False):
    """Frame, size and status of every chunk from single-level handles through the existing device
    entry: one call per distinct level over that level's chunks, the same max_chunk."""
    max_chunk = max_chunk or max(max(len(d) for d in datas), 1)
    frames, sizes, st = [None] * len(datas), [None] * len(datas), [None] * len(datas)
    for lv in sorted(set(levels)):
        idx = [i for i, v in enumerate(levels) if v == lv]
        f, s, t, _ = run([datas[i] for i in idx], level=lv, max_chunk=max_chunk, checksum=checksum)
        for k, i in enumerate(idx):
            frames[i], sizes[i], st[i] = f[k], s[k], t[k]
    return frames, sizes, st


@functools.lru_cache(maxsize=None)
def batch():
    """The shared interleaved batch: 24 chunks of five kinds, the edge sizes among them, levels
    cycling through CYCLE so that no parse class is contiguous in input order -> (chunks, levels,
    oracle frames).  Read-only."""
    sizes = [65536, 1, 5, 4096, 65535, 65536, 300, 20000, 40001, 65536, 4096, 65535, 65536, 1000, 65536, 5, 12345, 65536, 65535, 64, 65536,
             30000, 1, 65536]
    kinds = [T.DG_TEXT, T.DG_JSON, T.DG_MIX, T.DG_RANDOM, None]
    datas = []
    for i, n in enumerate(sizes):
        k = kinds[i % 5]
        datas.append(np.zeros(n, np.uint8) if k is None else T.gen(k, 1, 0x5EED0B00 + i, n))
    levels = [CYCLE[i % len(CYCLE)] for i in range(len(sizes))]
    assert {1, 5, 4096, 65535, 65536} <= set(sizes) and set(levels) == set(CYCLE)
    classes = [parse_class(v) for v in levels]
    assert set(classes) == set(range(9))
    for c in range(9):  # no class is one contiguous run of the input
        idx = [i for i, v in enumerate(classes) if v == c]
        assert idx[-1] - idx[0] + 1 > len(idx)
    return datas, levels, [T.oracle_frame(d, level=lv) for d, lv in zip(datas, levels)]


def check_decodes(frames, datas):
    for i, (f, d) in enumerate(zip(frames, datas)):
        assert T.zstd_decompress(f, len(d)) == d.tobytes(), i


def test_every_class_interleaved(libzstd):
    datas, levels, want = batch()
    frames, sizes, st, _ = run(datas, levels)
    ref, ref_sizes, ref_st = single_level_frames(datas, levels)
    assert st == [0] * len(datas) == ref_st
    assert sizes == ref_sizes == [len(w) for w in want]
    for i, (f, w, r) in enumerate(zip(frames, want, ref)):
        assert f == w, (i, levels[i], "oracle")
        assert f == r, (i, levels[i], "single-level handle")
    check_decodes(frames, datas)


@pytest.mark.parametrize("level", [1, 2, 3, 9])
def test_one_level_for_all(libzstd, level):
    """One class holds everything and every other range is empty."""
    datas = batch()[0][:9]
    frames, sizes, st, _ = run(datas, [level] * len(datas))
    ref, ref_sizes, ref_st = run(datas, level=level)[:3]
    assert (frames, sizes, st) == (ref, ref_sizes, ref_st) and st == [0] * len(datas)
    check_decodes(frames, datas)


@pytest.mark.parametrize("where", ["first", "last"])
def test_class_of_one_item(libzstd, where):
    """A class holding exactly one item, at index 0 / at the last index, the rest at level 3."""
    datas = batch()[0][:8]
    for lone in (1, 12):  # a K1 class in front of level 3's, a deep class behind it
        levels = [3] * len(datas)
        levels[0 if where == "first" else -1] = lone
        frames, sizes, st, _ = run(datas, levels)
        assert st == [0] * len(datas)
        for i, (f, d, lv) in enumerate(zip(frames, datas, levels)):
            assert f == T.oracle_frame(d, level=lv), (lone, i)
        check_decodes(frames, datas)


def test_count_one_and_zero(libzstd):
    import torch

    import cuda_zstd

    d = batch()[0][0]
    for lv in (2, 7):
        frames, sizes, st, _ = run([d], [lv])
        assert st == [0] and frames[0] == T.oracle_frame(d, level=lv) == run([d], level=lv)[0][0]
    bc = cuda_zstd.BatchedCompressor(3)
    empty = torch.zeros(0, dtype=torch.int64, device="cuda")
    L = cuda_zstd.lib()
    assert L.nvcomp_zstd_batched_compress_levels_async_v5(bc._h, None, None, None, 65536, 0, None, None, None, None, 0, None) == 0
    bc.compress_levels_async(empty, empty, torch.zeros(0, dtype=torch.int32, device="cuda"), 65536, empty, empty, None, empty.view(torch.uint8))
    torch.cuda.synchronize()
    bc.close()


def heavy_draw(heavy):
    """300 levels from the selector's eight, seeded: nine in ten from the levels of one parse class
    (`heavy`), the rest uniform over the others, so that class holds more items than the 256
    persistent workgroups of a launch and every other class fewer."""
    rng = np.random.default_rng(0x5EED0B03)
    rest = [v for v in SELECTOR_LEVELS if v not in heavy]
    return [int(rng.choice(heavy)) if rng.random() < 0.9 else int(rng.choice(rest)) for _ in range(300)]


@pytest.mark.parametrize("heavy", [(3,), (12, 16, 19)], ids=["k1", "deep"])
def test_ranges_against_the_persistent_loop(libzstd, heavy):
    """300 chunks of 4 KiB: a launch has min(300, CUs) = 256 workgroups, so the heavy class (over
    256 items: its workgroups come back to the counter for a second block) and the light ones
    (most workgroups find the range exhausted at once) both run.  Once with K1's level-3 class
    heavy, once with the deep matcher's depth-128 class (levels 12, 16 and 19)."""
    levels = heavy_draw(list(heavy))
    counts = np.bincount([parse_class(v) for v in levels], minlength=9)
    assert counts.max() > 256 and counts[parse_class(heavy[0])] == counts.max()
    assert sum(1 for c in counts if 0 < c < 256) >= 3
    data = T.gen(T.DG_MIX, 300, 0x5EED0B04, 4096)
    datas = [data[i * 4096:(i + 1) * 4096] for i in range(300)]
    frames, sizes, st, _ = run(datas, levels)
    assert st == [0] * 300
    for i, (f, d, lv) in enumerate(zip(frames, datas, levels)):
        assert f == T.oracle_frame(d, level=lv), (i, lv)


def test_multi_block_frames(libzstd):
    """max_chunk of 160 KiB (five 32 KiB history blocks per item, staged and gathered): every
    frame equals the oracle's at its level's window log."""
    sizes = [163840, 70 * 1024, 65537, 10]
    datas = [T.gen(k, 1, 0x5EED0B05 + i, n) for i, (k, n) in enumerate(zip([T.DG_TEXT, T.DG_JSON, T.DG_MIX, T.DG_TEXT], sizes))]
    seen = set()
    for levels in ([1, 3, 9, 12], [12, 9, 3, 1], [9, 12, 1, 3], [3, 1, 12, 9]):  # every size at every level
        frames, out_sizes, st, _ = run(datas, levels, max_chunk=163840)
        assert st == [0] * 4
        for i, (f, d, lv) in enumerate(zip(frames, datas, levels)):
            assert f == T.oracle_frame(d, level=lv), (i, lv)
            if not (f[4] >> 5) & 1:  # not a single-segment frame: the Window_Descriptor is the level's own
                assert f[5] == (T.level_window_log(lv) - 10) << 3
                seen.add(f[5])
        check_decodes(frames, datas)
    assert len(seen) == 4


@pytest.mark.parametrize("bad", [0, 23, -1])
def test_invalid_level(libzstd, bad):
    datas, levels, want = batch()
    levels = list(levels)
    k = 11
    levels[k] = bad
    frames, sizes, st, raw = run(datas, levels)
    assert st[k] == 2 and sizes[k] == 0 and bool((raw[k] == SENTINEL).all())
    for i in range(len(datas)):
        if i != k:
            assert st[i] == 0 and frames[i] == want[i], i


def test_checksum_handle(libzstd):
    datas, levels, _ = batch()
    datas, levels = datas[:12], levels[:12]
    frames, sizes, st, _ = run(datas, levels, checksum=True)
    assert st == [0] * 12
    for i, (f, d, lv) in enumerate(zip(frames, datas, levels)):
        assert f == T.oracle_frame(d, checksum=True, level=lv), (i, lv)
    check_decodes(frames, datas)  # libzstd verifies the checksum


def test_refusals(libzstd):
    import torch

    import cuda_zstd

    datas, levels, _ = batch()
    datas, levels = datas[:6], levels[:6]
    bc = cuda_zstd.BatchedCompressor(3)
    n, cs = len(datas), 65536
    slot = (bc.max_out(cs) + 255) // 256 * 256
    ins = [torch.from_numpy(d).cuda() for d in datas]
    out = torch.full((n * slot,), SENTINEL, dtype=torch.uint8, device="cuda")
    ptrs = torch.tensor([t.data_ptr() for t in ins], dtype=torch.int64, device="cuda")
    optr = torch.tensor([out.data_ptr() + i * slot for i in range(n)], dtype=torch.int64, device="cuda")
    isz = torch.tensor([len(d) for d in datas], dtype=torch.int64, device="cuda")
    osz = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    dl = torch.tensor(levels, dtype=torch.int32, device="cuda")
    temp = torch.empty(bc.temp_size_levels(n, cs) - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(cuda_zstd.ZstdError) as e:
        bc.compress_levels_async(ptrs, isz, dl, cs, optr, osz, st, temp)
    torch.cuda.synchronize()
    assert e.value.code == 7
    assert bool((out == SENTINEL).all()) and bool((osz == -7).all()) and bool((st == -1).all())
    full = torch.empty(bc.temp_size_levels(n, cs), dtype=torch.uint8, device="cuda")
    with pytest.raises(cuda_zstd.ZstdError) as e:  # null d_levels
        bc.compress_levels_async(ptrs, isz, None, cs, optr, osz, st, full)
    assert e.value.code == 2
    with pytest.raises(cuda_zstd.ZstdError) as e:  # max_chunk == 0
        bc.compress_levels_async(ptrs, isz, dl, 0, optr, osz, st, full)
    assert e.value.code == 2
    bc.set_dictionary(cuda_zstd.Dictionary.load(T.gen(T.DG_JSON, 1, 0x5EED0B06, 16384).tobytes()))
    with pytest.raises(cuda_zstd.ZstdError) as e:  # a handle with a dictionary
        bc.compress_levels_async(ptrs, isz, dl, cs, optr, osz, st, full)
    torch.cuda.synchronize()
    assert e.value.code == 2
    assert bool((out == SENTINEL).all()) and bool((osz == -7).all())
    bc.close()


def test_stream_order_after_analysis(libzstd):
    """analyze_batch_device, then compress_levels_async fed its level tensor, on a side stream
    with no synchronise in between: the frames are compress_batch_adaptive's."""
    import torch

    import cuda_zstd

    datas = [batch()[0][i] for i in (0, 1, 2, 3, 4, 9, 13, 17, 20, 21)] + [np.zeros(65536, np.uint8), T.gen(T.DG_RANDOM, 1, 0x5EED0B07, 65536)]
    n, cs = len(datas), 65536
    chunks = [torch.from_numpy(np.ascontiguousarray(d)).cuda() for d in datas]
    bc = cuda_zstd.BatchedCompressor(3)
    slot = (bc.max_out(cs) + 255) // 256 * 256
    out = torch.full((n * slot,), SENTINEL, dtype=torch.uint8, device="cuda")
    ptrs = torch.tensor([t.data_ptr() for t in chunks], dtype=torch.int64, device="cuda")
    optr = torch.tensor([out.data_ptr() + i * slot for i in range(n)], dtype=torch.int64, device="cuda")
    isz = torch.tensor([len(d) for d in datas], dtype=torch.int64, device="cuda")
    osz = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    temp = torch.empty(bc.temp_size_levels(n, cs), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    d_levels, _ = cuda_zstd.analyze_batch_device(ptrs, isz, cuda_zstd.BALANCED, 65536, stream=side)
    bc.compress_levels_async(ptrs, isz, d_levels, cs, optr, osz, st, temp, stream=side)
    side.synchronize()
    sizes, host = osz.cpu().tolist(), out.cpu().numpy()
    assert st.cpu().tolist() == [0] * n
    want, levels = cuda_zstd.compress_batch_adaptive(chunks, cuda_zstd.BALANCED)
    torch.cuda.synchronize()
    assert levels == d_levels.cpu().tolist() and len(set(levels)) >= 3
    for i, w in enumerate(want):
        assert host[i * slot:i * slot + sizes[i]].tobytes() == w.cpu().numpy().tobytes(), (i, levels[i])
    bc.close()


def test_python_surface(libzstd):
    import torch

    import cuda_zstd

    datas, levels, want = batch()
    chunks = [torch.from_numpy(d).cuda() for d in datas]
    by_list = cuda_zstd.compress_batch_levels(chunks, levels)
    by_tensor = cuda_zstd.compress_batch_levels(chunks, torch.tensor(levels, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert [f.cpu().numpy().tobytes() for f in by_list] == want
    assert [f.cpu().numpy().tobytes() for f in by_tensor] == want
    assert cuda_zstd.compress_batch_levels([], []) == []
    with pytest.raises(cuda_zstd.ZstdError):
        cuda_zstd.compress_batch_levels(chunks[:3], [3, 0, 3])

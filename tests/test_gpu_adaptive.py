"""Adaptive level selection on the GPU (csrc/zh_adaptive.hip) against the numpy model
(tests/zh_adaptive_model.py).

Integer statistics (repeated_pairs, max_run_length, pattern_score, unique_bytes, sample_size, and
the histogram read from the temp records) are compared exactly.  fp32 derived values are within
2e-4 of the fp64 model (the bound worked out in tests/test_adaptive_host.py; the device's tree sum
is tighter).  Levels and flags are compared where the model keeps its margin from the rule's
thresholds; every case here keeps it except DG_SOURCE (compressibility 0.398: integers only).
Two zeros are compared too: their repetition ratio is exactly 1/2 in fp32 and fp64 alike.

The cases are analysed as a few batches, once per module, and shared by the tests."""
import ctypes
import functools

import numpy as np
import pytest

import zh_adaptive_model as M
import zh_testlib as T

pytestmark = pytest.mark.gpu
TOL = 2e-4
SEED = M.SEED
HOST_NAMES, host_inputs = M.NAMES, M.named_inputs
SIZES = [1, 2, 4, 5, 8, 9, 63, 64, 65, 255, 256, 257, 16383, 16384, 16385, 65535, 65536]
INT_FIELDS = ("repeated_pairs", "max_run_length", "pattern_score", "unique_bytes")


class Case:
    def __init__(self, name, data, offset=0, levels=True):
        self.name, self.data, self.offset, self.levels = name, np.ascontiguousarray(data), offset, levels


@functools.lru_cache(maxsize=None)
def groups():
    """sample_bytes -> cases.  The 64 KiB group is the mixed batch: sizes 0 .. 65536, every input
    kind, misaligned bases."""
    rng = np.random.default_rng(0x5EED0A02)
    text = T.gen(T.DG_TEXT, 1, SEED, 65536)
    mix = T.gen(T.DG_MIX, 1, SEED, 65536)
    main = [Case(k, host_inputs()[k]) for k in HOST_NAMES]
    main.append(Case("SOURCE", T.gen(T.DG_SOURCE, 1, SEED, 65536), levels=False))
    main.append(Case("empty", np.zeros(0, np.uint8)))
    for n in SIZES:
        main.append(Case(f"zeros_{n}", np.zeros(n, np.uint8)))
        main.append(Case(f"text_{n}", text[:n]))
    # base pointers 1, 3 and 7 bytes into a tensor
    main += [Case("mix_off1", mix[:65528], 1), Case("mix_off3", mix[:20001], 3), Case("mix_off7", mix[:257], 7),
             Case("zeros_off3", np.zeros(40000, np.uint8), 3), Case("text_off7_9", text[:9], 7)]
    # runs of 256 and more across a tile edge (16384) and across a wave's 4 KiB, aligned and not
    main += [Case("run300_tile_edge", M.random_with_run(65536, 16384 - 100, 300)),
             Case("run300_tile_edge_off5", M.random_with_run(65536, 16384 - 100, 300), 5),
             Case("run256_wave_edge", M.random_with_run(20000, 4096 - 10, 256)),
             Case("run255_wave_edge", M.random_with_run(20000, 4096 - 250, 255)),
             Case("run257_last_tile", M.random_with_run(65536, 65536 - 257, 257))]
    # a 4096-byte sample of 64 KiB chunks whose bytes past it are one long run: nothing past the sample counts
    tail = rng.integers(0, 256, 65536, dtype=np.uint8)
    tail[4000:] = 7
    tail2 = rng.integers(0, 256, 65536, dtype=np.uint8)
    tail2[4096:] = tail2[4095]
    small = [Case("run_from_4000", tail), Case("run_from_4096", tail2), Case("run_from_4000_off3", tail, 3), Case("zeros", np.zeros(65536, np.uint8)),
             Case("text_100", text[:100])]
    # 160 KiB, sample 163840: runs across offset 65536
    big = [Case("run120_at_64k", M.random_with_run(163840, 65536 - 60, 120)), Case("run101_at_64k", M.random_with_run(163840, 65536 - 50, 101)),
           Case("run120_at_64k_off1", M.random_with_run(163840, 65536 - 60, 120), 1)]
    return {65536: main, 4096: small, 163840: big}


def device_chunks(cases):
    import torch

    out = []
    for c in cases:
        t = torch.zeros(len(c.data) + c.offset + 16, dtype=torch.uint8, device="cuda")
        v = t[c.offset : c.offset + len(c.data)]
        if len(c.data):
            v.copy_(torch.from_numpy(c.data))
        assert v.data_ptr() % 16 == c.offset
        out.append(v)
    return out


@functools.lru_cache(maxsize=None)
def gpu(sample_bytes, preference):
    """(levels, stats records) of a group from one analyze_batch call."""
    import cuda_zstd

    levels, stats = cuda_zstd.analyze_batch(device_chunks(groups()[sample_bytes]), preference, sample_bytes)
    return levels.cpu().numpy(), cuda_zstd.adaptive_stats_numpy(stats)


@functools.lru_cache(maxsize=None)
def model(sample_bytes, preference):
    return [M.analyze(c.data, preference, sample_bytes) for c in groups()[sample_bytes]]


def compare(sample_bytes, preference, with_levels):
    levels, stats = gpu(sample_bytes, preference)
    cases = groups()[sample_bytes]
    assert stats.dtype.itemsize == M.STATS_DTYPE.itemsize and len(stats) == len(levels) == len(cases)
    for i, (c, want) in enumerate(zip(cases, model(sample_bytes, preference))):
        got = stats[i]
        assert got["sample_size"] == want["n"], c.name
        for k in INT_FIELDS:
            assert got[k] == want[k], (c.name, k, int(got[k]), want[k])
        for k in ("entropy", "repetition_ratio", "compressibility"):
            assert abs(float(got[k]) - want[k]) <= TOL, (c.name, k, float(got[k]), want[k])
        assert levels[i] == got["level"], c.name
        if with_levels and c.levels:
            assert want["margin_ok"], c.name  # no case is left out
            assert int(got["flags"]) == (1 if want["has_patterns"] else 0) | (2 if want["is_random"] else 0), c.name
            assert levels[i] == want["level"], (c.name, int(levels[i]), want["level"])


@pytest.mark.parametrize("sample_bytes", [65536, 4096, 163840])
def test_batch_statistics(sample_bytes):
    compare(sample_bytes, M.BALANCED, with_levels=False)
    if sample_bytes == 163840:
        runs = {c.name: int(s["max_run_length"]) for c, s in zip(groups()[sample_bytes], gpu(sample_bytes, M.BALANCED)[1])}
        assert runs == {"run120_at_64k": 120, "run101_at_64k": 101, "run120_at_64k_off1": 120}
    if sample_bytes == 65536:
        st = {c.name: s for c, s in zip(groups()[sample_bytes], gpu(sample_bytes, M.BALANCED)[1])}
        assert st["run300_tile_edge"]["max_run_length"] == 256 and st["run300_tile_edge_off5"]["max_run_length"] == 256
        assert st["run255_wave_edge"]["max_run_length"] == 255
        assert [int(st[f"zeros_{n}"]["pattern_score"]) for n in (1, 4, 5, 8, 9)] == [0, 0, 1, 4, 7]
        e = st["empty"]
        assert e["level"] == 3 and all(int(e[k]) == 0 for k in INT_FIELDS + ("sample_size", "flags")) and e["entropy"] == 0 and e["compressibility"] == 0


@pytest.mark.parametrize("preference", [M.SPEED, M.BALANCED, M.RATIO])
def test_levels(preference):
    for sample_bytes in (65536, 4096, 163840):
        compare(sample_bytes, preference, with_levels=True)
    # all five branches, by the named inputs
    lv = {c.name: int(l) for c, l in zip(groups()[65536], gpu(65536, preference)[0])}
    assert [lv[k] for k in ("RANDOM", "zeros", "random_run300", "period50", "01", "TEXT")] == [M.LEVELS[b][preference] for b in (0, 1, 1, 2, 3, 4)]


def raw_call(cz, chunks, sample_bytes, preference, temp_bytes=None, stream=None, with_stats=True):
    """The C entry with caller-owned buffers -> (rc, levels, stats, temp) device tensors."""
    import torch

    n = len(chunks)
    ptrs = torch.tensor([c.data_ptr() for c in chunks], dtype=torch.int64).cuda()
    sizes = torch.tensor([c.numel() for c in chunks], dtype=torch.int64).cuda()
    need = cz.lib().cuda_zstd_adaptive_get_temp_size(n)
    temp = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")  # the entry zeroes it itself
    levels = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    stats = torch.zeros(n * 40, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = cz.lib().cuda_zstd_adaptive_analyze_batch_async(ptrs.data_ptr(), sizes.data_ptr(), n, sample_bytes, preference,
                                                         stats.data_ptr() if with_stats else None, levels.data_ptr(), temp.data_ptr(),
                                                         need if temp_bytes is None else temp_bytes,
                                                         stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    return rc, levels, stats, temp


def test_histogram_records_and_null_stats():
    import cuda_zstd as cz
    import torch

    cases = [c for c in groups()[65536] if c.name in ("MIX", "zeros", "text_16385", "mix_off3", "text_9", "empty", "run300_tile_edge_off5")]
    rc, levels, _, temp = raw_call(cz, device_chunks(cases), 65536, M.BALANCED, with_stats=False)
    assert rc == cz.OK
    torch.cuda.synchronize()
    rec = temp.cpu().numpy().view(np.uint32).reshape(len(cases), 259)
    for i, c in enumerate(cases):
        want = M.analyze(c.data)
        assert (rec[i, :256] == want["hist"]).all(), c.name
        assert list(rec[i, 256:]) == [want["repeated_pairs"], want["max_run_length"], want["pattern_score"]], c.name
        assert int(levels[i]) == want["level"], c.name


def test_repeatable_and_other_stream():
    import cuda_zstd as cz
    import torch

    chunks = device_chunks(groups()[65536])
    torch.cuda.synchronize()
    l1, s1 = cz.analyze_batch(chunks, M.RATIO)
    l2, s2 = cz.analyze_batch(chunks, M.RATIO)
    side = torch.cuda.Stream()
    l3, s3 = cz.analyze_batch(chunks, M.RATIO, stream=side)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(l1, l2) and torch.equal(s1, s2)
    assert torch.equal(l1, l3) and torch.equal(s1, s3)
    assert np.array_equal(l1.cpu().numpy(), gpu(65536, M.RATIO)[0])


def test_select_level_agrees_with_batch():
    import cuda_zstd as cz

    cases = groups()[65536]
    pick = [i for i, c in enumerate(cases) if c.name in ("MIX", "zeros", "period50", "text_257", "mix_off7", "zeros_2", "run300_tile_edge")]
    chunks = device_chunks([cases[i] for i in pick])
    for preference in (M.SPEED, M.BALANCED, M.RATIO):
        stats = gpu(65536, preference)[1]
        for i, t in zip(pick, chunks):
            got = cz.select_level(t, preference)
            for k in M.STATS_DTYPE.names:
                assert got[k] == stats[i][k], (cases[i].name, k)
    tail = next(c for c in groups()[4096] if c.name == "run_from_4000")
    got = cz.select_level(device_chunks([tail])[0], M.BALANCED, sample_bytes=4096)
    assert got["max_run_length"] == 96 and got["sample_size"] == 4096
    # host bytes are uploaded; is_compressible is the reference's > 0.3 and 1 + 3 c
    z = cz.select_level(bytes(70000))
    assert z["level"] == 12 and z["sample_size"] == 65536
    ok, ratio = cz.is_compressible(bytes(70000))
    assert ok and abs(ratio - 4.0) <= 3 * TOL
    ok, ratio = cz.is_compressible(host_inputs()["RANDOM"])
    assert not ok and abs(ratio - (1.0 + 3.0 * M.analyze(host_inputs()["RANDOM"])["compressibility"])) <= 3 * TOL


def test_error_codes_on_device_arguments():
    import cuda_zstd as cz
    import torch

    chunks = device_chunks(groups()[4096])
    need = cz.lib().cuda_zstd_adaptive_get_temp_size(len(chunks))
    rc, levels, _, temp = raw_call(cz, chunks, 4096, M.BALANCED, temp_bytes=need - 1)
    torch.cuda.synchronize()
    assert rc == cz.TOO_SMALL
    assert bool((levels == -1).all()) and bool((temp == 0xA5).all())  # nothing was launched
    L = cz.lib()
    d = temp.data_ptr()
    ok = (d, d, 1, 4096, 1, None, d, d, need, None)
    for pos, bad in ((0, None), (1, None), (6, None), (7, None), (7, d + 2), (3, 0), (4, 3), (4, -1)):
        args = list(ok)
        args[pos] = bad
        assert L.cuda_zstd_adaptive_analyze_batch_async(*args) == cz.INVALID, pos
    out = cz.AdaptiveStats()
    assert L.cuda_zstd_adaptive_select_level(None, 16, 65536, 1, ctypes.byref(out), None) == cz.INVALID
    assert L.cuda_zstd_adaptive_select_level(d, 0, 65536, 1, ctypes.byref(out), None) == cz.INVALID
    assert L.cuda_zstd_adaptive_select_level(d, 16, 65536, 7, ctypes.byref(out), None) == cz.INVALID
    with pytest.raises(cz.ZstdError):
        cz.select_level(b"")


def test_compress_batch_adaptive():
    import cuda_zstd as cz
    import torch

    names = ["RANDOM", "zeros", "period50", "01", "TEXT", "JSON", "MIX", "0123", "random_run300", "SYM16", "CSV", "SENSOR"]
    chunks = [host_inputs()[k] for k in names]
    frames, levels = cz.compress_batch_adaptive([torch.from_numpy(c).cuda() for c in chunks], M.BALANCED)
    torch.cuda.synchronize()
    assert levels == [M.analyze(c)["level"] for c in chunks]
    assert len(set(levels)) >= 3 and len(frames) == 12
    for name, c, f, lv in zip(names, chunks, frames, levels):
        got = f.cpu().numpy().tobytes()
        assert got == T.oracle_frame(c, level=lv), (name, lv)
        assert T.zstd_decompress(got, len(c)) == c.tobytes(), name

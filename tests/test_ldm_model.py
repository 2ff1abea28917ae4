"""Long-distance matching without a GPU: the numpy model's frames (zh_ldm_model.py) through libzstd
for the inputs the GPU tests use (zh_ldm_inputs.py), the size bounds those tests assert checked on
the model's partition alone, the model's own rules, and csrc/zh_ldm.h under sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import zh_ldm_inputs as I
import zh_ldm_model as M
import zh_testlib as T

KIB = 1024
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(I.SMALL))
def test_model_frame_decodes(libzstd, name):
    """Raw blocks for the gaps, one-sequence blocks for the runs: libzstd gives the input back."""
    data, wl, hl = I.SMALL[name]()
    rec = M.plan(data, wl, hl)
    parts = M.partition(len(data), rec)
    assert sum(p[2] for p in parts) == len(data) and all(p[2] > 0 for p in parts)
    assert all(p[2] >= M.MIN_SEG and M.MIN_DIST < p[3] <= M.max_dist(wl) and p[3] <= p[1] for p in parts if p[0] == "ldm")
    assert not rec[0].any()  # cell 0 is never split
    assert T.zstd_decompress(M.model_frame(data, parts, wl), len(data)) == data.tobytes()


def test_distance_just_under_2_27(libzstd):
    """Offset code 26 at its top: a 40,000-byte repeat 2^27 - 5 bytes back, window 2^27.  The run
    starts 5 bytes before a cell boundary, so its first block has match length 5."""
    d = (1 << 27) - 5
    rep = np.random.default_rng(5).integers(0, 256, 40000, dtype=np.uint8)
    data = np.zeros(d + len(rep), np.uint8)
    data[: len(rep)] = rep
    data[d:] = rep
    rec = np.zeros(((len(data) + M.CELL - 1) // M.CELL, 3), np.uint32)
    at = d
    while at < len(data):
        c = at // M.CELL
        ln = min(len(data), (c + 1) * M.CELL) - at
        rec[c] = (at, ln, d)
        at += ln
    parts = M.partition(len(data), rec)
    assert [p[2] for p in parts if p[0] == "ldm"] == [5, 32768, 7227]
    frame = M.model_frame(data, parts, 27)
    assert T.zstd_decompress(frame, len(data)) == data.tobytes()


def test_case1_bound_holds_for_the_partition():
    """test_gpu_ldm's case 1 bound, len(on) <= len(off) - 96 KiB + 16 x 5 + 2 x 1100, assumes at
    most 5 one-sequence blocks of at most 16 bytes that cover the second A up to 1100 bytes a side."""
    data, wl, hl = I.case1()
    parts = M.partition(len(data), M.plan(data, wl, hl))
    saved, nblk = M.saved_bytes(parts)
    assert nblk <= 5 and saved >= 96 * KIB - 2 * 1100
    assert max(len(M.ldm_block(p[2], p[3], False)) for p in parts if p[0] == "ldm") <= M.BLOCK_MAX


def test_case10_model_and_bound():
    """The model on case 10's 16 MiB (one run of it, about 9 s): every cell of the second half is one
    block of 32 KiB at distance 2^23 and the first half is not split -- the closed form
    test_gpu_ldm compares the finder with.  Its bound, len(on) <= len(first half alone) + 16 x 256 +
    2 KiB, then holds for the partition: 256 one-sequence blocks of at most 16 bytes, the first
    half's blocks unchanged."""
    data, wl, hl = I.case10()
    rec = M.plan(data, wl, hl)
    assert (rec == I.case10_records()).all()
    parts = M.partition(len(data), rec)
    ldm = [p for p in parts if p[0] == "ldm"]
    assert len(ldm) == 256 and sum(p[2] for p in ldm) == len(data) // 2
    assert [p for p in parts if p[1] < len(data) // 2] == [("gap", c * M.CELL, M.CELL) for c in range(256)]
    assert max(len(M.ldm_block(p[2], p[3], k + 1 == len(ldm))) for k, p in enumerate(ldm)) <= M.BLOCK_MAX


def test_block_is_at_most_16_bytes():
    for ml in (3, 130, 131, M.MIN_SEG, 32768):
        for dist in (32769, 100000, (1 << 27) - 5, M.MAX_DIST):
            assert len(M.ldm_block(ml, dist, True)) <= M.BLOCK_MAX


def test_hash_covers_exactly_64_bytes():
    rng = np.random.default_rng(9)
    a = rng.integers(0, 256, 300, dtype=np.uint8)
    b = a.copy()
    b[99] ^= 1  # positions 36..99 see it
    ha, hb = M.hashes(a), M.hashes(b)
    diff = np.flatnonzero(ha != hb)
    assert diff.tolist() == list(range(36, 100))
    assert M.hash_at(a, 17) == int(ha[17])
    assert len(set(M.G.tolist())) == 256


def test_sample_rate_and_cell_cap():
    data = np.random.default_rng(10).integers(0, 256, 4 * M.CELL, dtype=np.uint8)
    pos, h = M.kept_samples(data)
    assert 0.6 * len(data) / 128 < len(pos) < 1.4 * len(data) / 128  # one position in 2^RATE_LOG
    assert M.is_sample(h).all() and pos.max() + M.HASH_BYTES <= len(data)
    data, _, _ = I.case7("sampled-byte")  # every position is a sample: the first 512 of each cell stay
    pos, _ = M.kept_samples(data)
    want = np.concatenate([np.arange(c * M.CELL, c * M.CELL + M.CELL_SAMPLES) for c in range(len(data) // M.CELL)])
    assert (pos == want).all()


def test_table_keeps_the_earliest_position():
    pos = np.array([50, 10, 30], dtype=np.int64)
    h = np.array([7, 7, 7], dtype=np.uint64)
    table = M.build_table(pos, h, 10)
    e = int(table[M.slot_of(h[:1], 10)[0]])
    assert e >> 32 == 10 and e & 0xFFFFFFFF == int(M.tag_of(h[:1])[0])
    assert int((table != np.uint64(M.M64)).sum()) == 1


def test_longest_run_ties_go_to_the_lowest_start():
    eq = np.array([0, 1, 1, 1, 0, 1, 1, 1, 0, 1], bool)
    assert M.longest_run(eq) == (1, 3)
    assert M.longest_run(np.zeros(5, bool)) == (0, 0)
    assert M.longest_run(np.ones(5, bool)) == (0, 5)


@pytest.mark.parametrize("kind", ["longer", "six", "equal"])
def test_offset_rules(kind):
    data, wl, hl, want = I.case5(kind)
    rec = M.plan(data, wl, hl)
    assert [tuple(int(v) for v in r) for r in rec if r[1]] == [want]


def test_table_log_rule():
    assert M.table_log(65537, 20) == 11 and M.table_log(1 << 20, 20) == 14 and M.table_log(1 << 20, 10) == 10
    assert M.table_log((1 << 20) + 1, 20) == 15 and M.table_log(1 << 32, 20) == 20


def test_header_under_sanitizers(tmp_path):
    """tests/cpp/ldm_block_check.cpp (its own main) built with ASan + UBSan, runtimes linked into
    the program: csrc/zh_ldm.h's block writer, hash, predicate, slot, tag and table size against
    tests/golden/ldm_blocks.json."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "ldm_block_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-I", os.path.join(ROOT, "custom-nvcomp-with-zstd_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "ldm_block_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, os.path.join(T.GOLDEN, "ldm_blocks.json")], capture_output=True, text=True)
    assert r.returncode == 0 and "ldm OK" in r.stdout, r.stdout + r.stderr


def test_capi_arguments_and_workspace_sizes():
    """cuda_zstd_set_long_distance: with enable set 0 selects window 27 / table 20, a window outside
    16..31 is refused with 2; the workspace grows only with the flag set and only for frames the plan applies
    to (no GPU needed: sizes are host arithmetic)."""
    import cuda_zstd

    lib = cuda_zstd.lib()
    m = cuda_zstd.Manager(3)
    n = 236609
    before = [m.workspace_size(k) for k in (1000, 65536, 65537, n, 16 << 20)]
    for wl in (15, 32, 9):
        assert lib.cuda_zstd_set_long_distance(m._h, 1, wl, 0) == 2
    assert lib.cuda_zstd_set_long_distance(m._h, 0, 15, 0) == 2
    assert [m.workspace_size(k) for k in (1000, 65536, 65537, n, 16 << 20)] == before  # a refused call changes nothing
    assert lib.cuda_zstd_set_long_distance(m._h, 0, 20, 0) == 0
    assert [m.workspace_size(k) for k in (1000, 65536, 65537, n, 16 << 20)] == before
    assert lib.cuda_zstd_set_long_distance(m._h, 1, 0, 0) == 0
    after = [m.workspace_size(k) for k in (1000, 65536, 65537, n, 16 << 20)]
    assert after[:2] == before[:2] and all(a > 2 * b for a, b in zip(after[2:], before[2:]))
    assert lib.cuda_zstd_set_long_distance(m._h, 0, 0, 0) == 0  # off again; 0 leaves the window (27 by now) alone
    assert [m.workspace_size(k) for k in (1000, 65536, 65537, n, 16 << 20)] == before
    w27 = cuda_zstd.Manager(3)
    assert lib.cuda_zstd_set_long_distance(w27._h, 0, 27, 0) == 0
    assert lib.cuda_zstd_set_long_distance(None, 1, 0, 0) == 2
    zero = cuda_zstd.Manager(3, long_distance=0)  # 0 is off, not "the default window"
    assert [zero.workspace_size(k) for k in (65537, n)] == [before[2], before[3]]
    with pytest.raises(cuda_zstd.ZstdError):
        cuda_zstd.Manager(3, long_distance=12)

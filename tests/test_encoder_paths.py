"""Coverage proof of the compressor's entropy stage, on the CPU: the oracle frames of the
directed inputs (tests/zh_edge_inputs.py), walked by tests/zh_frames.py, reach every path the
encoder can emit, at each of the levels the GPU test runs (tests/test_gpu_encoder_paths.py
compresses the same inputs on the GPU and requires the same frames).  libzstd pins the oracle:
every frame decodes to its input.  A census of the repeat-offset cases (RFC 8878 §3.1.2.5) over
the level-3 parses does the same for the offset-code resolution."""
import ctypes

import numpy as np
import pytest

import zh_edge_inputs as E
import zh_frames as F
import zh_testlib as T

# every key of zh_frames.features() that the encoder can emit
ENCODER_PATHS = {
    "block_compressed", "block_raw", "block_rle",
    "lit_raw", "lit_rle", "lit_huffman", "lit_raw_h1", "lit_raw_h2", "lit_raw_h3", "lit_rle_h2", "lit_rle_h3",
    "lit_huf_h3", "lit_huf_h4", "lit_huf_h5", "huf_1stream", "huf_4stream", "weights_direct", "weights_fse",
    "huf_1stream_weights_direct", "huf_1stream_weights_fse", "huf_4stream_weights_direct", "huf_4stream_weights_fse",
    "nseq_bytes1", "nseq_bytes2", "no_sequences",
    "ll_predefined", "ll_rle", "ll_fse", "of_predefined", "of_rle", "of_fse", "ml_predefined", "ml_rle", "ml_fse",
}
# paths of the format the encoder never reaches, at any level
NEVER = {
    "nseq_bytes3": "a block carries at most 64 KiB of input and a match at least 5 bytes: fewer than 0x7F00 sequences",
    "lit_rle_h1": "up to 63 literals are never compressed (ZH_COMPRESS_LITERALS_SIZE_MIN), so RLE literals take 2 or 3 header bytes",
    "lit_treeless": "the encoder writes a Huffman table with every compressed literals section",
    "lit_treeless_h3": "as lit_treeless", "lit_treeless_h4": "as lit_treeless", "lit_treeless_h5": "as lit_treeless",
    "ll_repeat": "blocks are compressed independently: no table is carried from one to the next",
    "of_repeat": "as ll_repeat", "ml_repeat": "as ll_repeat",
}
# paths left out at one level: {level: {path: reason}}
RLE_H3 = ("4096 equal literals need 4096 matches of 5-7 bytes in a 32 KiB block with no match missed; the only source that gives them is "
          "the block before (builder `pieces`, pieces of 5, 6 and 7 bytes, seeds 1-6 searched), and the 2^14-entry tables of levels 1-3 "
          "and level 5's 4-step chains lose some of its 32 Ki positions")
LEVEL_ALLOW = {1: {"lit_rle_h3": RLE_H3}, 2: {"lit_rle_h3": RLE_H3}, 3: {"lit_rle_h3": RLE_H3}, 5: {"lit_rle_h3": RLE_H3}, 9: {}}


def required(level):
    return ENCODER_PATHS - set(LEVEL_ALLOW[level])


_frames = {}


def oracle_frames(level):
    """{name: (input, oracle frame)} of the level, made once."""
    if level not in _frames:
        _frames[level] = {n: (d, T.oracle_frame(d, level=level)) for n, d in E.cases(level)}
    return _frames[level]


def test_cases_are_small_and_deterministic():
    a, b = E.cases(3), E.cases(9)
    assert [n for n, _ in a] == [n for n, _ in b] and len({n for n, _ in a}) == len(a)
    for (n, x), (_, y) in zip(a, b):
        assert x.dtype == np.uint8 and 0 < len(x) <= 128 * 1024 and x.tobytes() == y.tobytes(), n
    assert sum(len(x) <= 10 * 1024 for _, x in a) > len(a) // 2


def test_allowlists_are_disjoint_from_what_is_required():
    assert not (ENCODER_PATHS & set(NEVER))
    for level in E.LEVELS:
        assert set(LEVEL_ALLOW[level]) <= ENCODER_PATHS and all(LEVEL_ALLOW[level].values())


@pytest.mark.parametrize("level", E.LEVELS)
def test_oracle_frames_decode_with_libzstd(libzstd, level):
    for n, (d, fr) in oracle_frames(level).items():
        assert T.zstd_decompress(fr, len(d)) == d.tobytes(), n


@pytest.mark.parametrize("level", E.LEVELS)
def test_cases_reach_every_encoder_path(level):
    fr = oracle_frames(level)
    got = F.features([f for _, f in fr.values()])
    assert got >= required(level), sorted(required(level) - got)
    assert not (got & set(NEVER)), sorted(got & set(NEVER))  # (then the allowlist is wrong)
    assert not (got & set(LEVEL_ALLOW[level])), sorted(got & set(LEVEL_ALLOW[level]))


def test_rle_literals_h3_search_finds_none_where_allowlisted():
    """The bounded search behind LEVEL_ALLOW: at the levels that leave lit_rle_h3 out, no seed 1-6
    of the `pieces` builders gives a block of RLE literals with the 3-byte header (level 9, whose
    32-step chains miss no piece, does: cases "rle_lits_4679" and "rle_lits_5458")."""
    for level in E.LEVELS:
        hits = [(b, s) for b in ("pieces5", "pieces6", "pieces7") for s in range(1, 7)
                if "lit_rle_h3" in F.features([T.oracle_frame(E.build(b, s), level=level)])]
        assert bool(hits) == ("lit_rle_h3" not in LEVEL_ALLOW[level]), (level, hits)


@pytest.mark.parametrize("level", E.LEVELS)
def test_size_boundaries(level):
    """The literal count on both sides of every boundary of the literals header, the sequence
    count on both sides of 128, and two sequences with one code each (predefined, not RLE)."""
    fr = oracle_frames(level)
    blocks = {n: F.walk(f) for n, (_, f) in fr.items()}
    lits = {(b["lit"], b["lit_hdr"], b["lit_n"], b.get("streams")) for w in blocks.values() for b in w if b["type"] == "compressed"}
    want = {("raw", 1, 31, None), ("raw", 2, 32, None), ("raw", 2, 63, None), ("huffman", 3, 64, 1), ("huffman", 3, 255, 1),
            ("huffman", 3, 256, 4), ("huffman", 3, 1023, 4), ("huffman", 4, 1024, 4), ("raw", 2, 4095, None), ("raw", 3, 4096, None),
            ("huffman", 4, 4095, 4), ("huffman", 4, 4096, 4), ("huffman", 4, 16383, 4), ("huffman", 5, 16384, 4), ("raw", 3, 16383, None),
            ("raw", 3, 16384, None)}
    assert {x[2] for x in want} == set(E.LITERAL_BOUNDARIES)
    assert lits >= want, sorted(want - lits, key=str)
    nseq = {(b["nseq"], b["nseq_bytes"]) for w in blocks.values() for b in w if b["type"] == "compressed"}
    assert {(127, 1), (128, 2), (1, 1), (0, 1)} <= nseq
    (two,) = blocks["two_same_codes"]
    assert two["nseq"] == 2 and two["modes"] == ("predefined", "predefined", "predefined")
    (three,) = blocks["all_rle"]
    assert three["nseq"] > 2 and three["modes"] == ("rle", "rle", "rle")


# ---- repeat offsets (level 3: orc_lz_parse is the level-3 parse)
REP_CASES = ("rep0", "rep1", "rep2", "rep1_ll0", "rep2_ll0", "rep0m1_ll0")
REP_ALLOW = {}  # case -> reason, for a case no seeded input reaches


def lz_parse(buf, pre):
    """The oracle's level-3 sequences [(ll, ml, off)] of buf[pre:] with buf[:pre] as history."""
    O = T.oracle()
    O.orc_lz_parse_pre.restype = ctypes.c_size_t
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    seq = np.zeros((len(buf) // 5 + 2, 3), np.uint32)
    last = ctypes.c_uint32(0)
    ns = O.orc_lz_parse_pre(buf.ctypes.data_as(T.vp), ctypes.c_uint32(pre), ctypes.c_uint32(len(buf)), seq.ctypes.data_as(T.vp), ctypes.byref(last))
    return [tuple(int(x) for x in s) for s in seq[:ns]]


def rep_census(seqs, rep, count):
    """RFC 8878 §3.1.2.5 restated: which repeat offset (if any) each sequence's offset is, and
    the history update.  rep entries of 0 are unknown (a block after the first) and never hit."""
    r = list(rep)
    for ll, _, off in seqs:
        cand = (("rep0", r[0]), ("rep1", r[1]), ("rep2", r[2])) if ll else (("rep1_ll0", r[1]), ("rep2_ll0", r[2]), ("rep0m1_ll0", r[0] - 1 if r[0] > 1 else 0))
        hit = next((k for k, (_, v) in enumerate(cand) if v and v == off), None)
        if hit is None:
            r = [off, r[0], r[1]]
            continue
        count[cand[hit][0]] = count.get(cand[hit][0], 0) + 1
        idx = hit + (0 if ll else 1)  # 0: rep0 (no change), 1: swap, 2: rotate, 3: rep0 - 1 pushed
        r = r if idx == 0 else [r[1], r[0], r[2]] if idx == 1 else [r[2], r[0], r[1]] if idx == 2 else [off, r[0], r[1]]
    return r


def test_repeat_offset_census_level_3():
    count, later_block_hits = {}, 0
    for n, (d, fr) in oracle_frames(3).items():
        blocks = F.walk(fr)
        bs = 65536 if len(d) <= 65536 else 32768  # (ZH_FRAME_BLOCK: larger frames are cut into 32 KiB blocks behind 32 KiB of history)
        assert len(blocks) == (len(d) + bs - 1) // bs, n
        for k, b in enumerate(blocks):
            if b["type"] != "compressed":
                continue
            pre = bs if k else 0
            seqs = lz_parse(d[k * bs - pre:(k + 1) * bs], pre)
            assert len(seqs) == b["nseq"], (n, k)
            before = sum(count.values())
            rep_census(seqs, (1, 4, 8) if k == 0 else (0, 0, 0), count)
            later_block_hits += (sum(count.values()) - before) if k else 0
    need = set(REP_CASES) - set(REP_ALLOW)
    assert {c for c in need if count.get(c, 0) > 0} == need, count
    # blocks after the first start with unknown history (cr0 = cr1 = cr2 = 0) and repeat offsets at once
    assert len(F.walk(oracle_frames(3)["rows_4_blocks"][1])) >= 3 and later_block_hits > 100, later_block_hits

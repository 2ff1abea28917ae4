"""The encoder's FSE chain by construction, on the CPU: the model of the chain kernel
(tests/zh_chain_model.py: the serial chain, and the 21-segment Jacobi scheme as k3_chain runs
it) traced over the oracle's level-3 parse of the directed inputs (tests/zh_chain_inputs.py).
The model checks itself (its stored states are the serial chain's), its tables are pinned to the
oracle's frames (modes and sequence count), libzstd pins those frames, and the census shows
that the inputs drive every table's chain through every named state of the scheme and put the
sequence count on both sides of every geometry edge.  tests/test_gpu_chain.py then requires the
GPU's frames of the same inputs to equal the oracle's: the census proves that the inputs force
the states, byte equality that the kernels handled them."""
import numpy as np
import pytest

import zh_chain_inputs as C
import zh_chain_model as M
import zh_testlib as T

# Tags no input can reach, with the reason; the census fails if one is ever met.
#   (table or "*", mode or "*", tag)
UNREACHABLE = {
    ("*", "*", "clamped"): "a live step's index is (s >> nb) + dFS of a symbol with a count: a state of that symbol, below 2^tableLog <= 512.  The "
                           "kernel's clamp is for dead steps, which may read a transform K2 never wrote (an RLE table has one) and whose result is dropped",
    ("*", "predefined", "rounds_max"): "the predefined ML table is taken when no code has nbSeq / 32 sequences; only codes 1-8 have more than one state "
                                       "in it, so three quarters of the steps map every state to one, and 20 rounds need 19 segments without such a step "
                                       "(LL and OF are not predefined on a chain of 321 sequences, the fewest with 21 live segments, or more: as below)",
    ("ll", "predefined", "long"): "nbSeq > 336 with every LL code below nbSeq / 32: at 337 sequences the 25 codes of fewer than 64 literals take 225, codes "
                                  "25-31 another 63, and 49 runs of 8,192 literals or more do not fit 64 KiB (more sequences need more)",
    ("of", "predefined", "long"): "a 64 KiB block has offset codes 0-15 only, so one of them has nbSeq / 16 sequences: never predefined from 32 sequences on",
}
# what every table reaches in FSE_Compressed mode, and the predefined ML table on a long chain
FSE_TAGS = tuple(t for t in M.TAGS if t != "clamped")
REQUIRED = {(t, "fse", g) for t in M.TABLES for g in FSE_TAGS} | {("ml", "predefined", "no_fixup"), ("ml", "predefined", "long")}
# one table in RLE mode beside two FSE tables, nbSeq > 336
MIXES = {("rle", "fse", "fse"), ("fse", "rle", "fse"), ("fse", "fse", "rle")}
# the widest 64-step append of the set (state bits + LL, ML and OF extra bits; DESIGN.md records it
# beside the sink's capacity), and the most sequences
WIDEST_CHUNK_BITS, MOST_SEQUENCES = 2026, 12483

_cache = {}


def traced():
    """{name: (input, oracle frame, trace)} of every case, made once"""
    if not _cache:
        for n, d in C.cases():
            _cache[n] = (d, T.oracle_frame(d, level=3), M.trace(d))  # (trace asserts segmented == serial)
    return _cache


def reached():
    got = set()
    for _, _, r in traced().values():
        for t in M.TABLES:
            x = r[t]
            got |= {(t, x["mode"], g) for g in x["tags"]}
            if x["nbSeq"] > 336:
                got.add((t, x["mode"], "long"))
    return got


def test_index_map_and_magic_exhaustive():
    """zh_k3_magic gives e / L by multiply-high for every L and every e < 2^14; the chain layout's
    index map is injective over a block's steps and tables and stays inside ZH_K3_BYTES / 3."""
    e = np.arange(1 << 14, dtype=np.uint64)
    for L in range(16, 1025, 16):
        m = M.k3_magic(L)
        g = ((e << np.uint64(8)) * np.uint64(m)) >> np.uint64(32)
        assert (g == e // np.uint64(L)).all(), L
        assert M.k3_index(L + 3, 1, L, m) == (0 * M.SLOTS + 3 * 1 + 1) * 16 + 3
        n = min(M.SEGS * L, 1 << 14)
        r = e[:n] - g[:n] * np.uint64(L)
        idx = np.concatenate([((r // np.uint64(16)) * np.uint64(M.SLOTS) + np.uint64(3) * g[:n] + np.uint64(t)) * np.uint64(16) + (r & np.uint64(15))
                              for t in range(3)])
        assert len(np.unique(idx)) == 3 * n, L
        # the layout of a block with L-step segments: 64 L state (u16) and 64 L code (u8) elements
        assert M.k3_bytes(M.SEGS * L) == 3 * M.SLOTS * L and int(idx.max()) < M.k3_bytes(M.SEGS * L) // 3, L
    for e1, t, L in ((0, 0, 16), (17, 2, 16), (13119, 2, 640), (16383, 1, 1024)):  # the scalar restatement agrees
        g, r = e1 // L, e1 % L
        assert M.k3_index(e1, t, L, M.k3_magic(L)) == ((r // 16) * 64 + 3 * g + t) * 16 + r % 16


def test_seglen_edges():
    assert [M.seglen(n) for n in (1, 336, 337, 672, 673, 2688, 2689, 13104, 13105, M.SEQ_CAP)] == [16, 16, 32, 32, 48, 128, 144, 624, 640, 640]


def test_cases_are_small_and_deterministic():
    a, b = C.cases(), C.cases()
    assert len({n for n, _ in a}) == len(a)
    for (n, x), (_, y) in zip(a, b):
        assert x.dtype == np.uint8 and 0 < len(x) <= 65536 and x.tobytes() == y.tobytes(), n


def test_model_checks_itself_and_matches_the_oracle_frames():
    """trace() asserted, per case and table, that the segmented scheme stored the serial chain's
    states and final state; its modes and sequence count are those of the oracle's frame."""
    for n, (_, fr, r) in traced().items():
        assert M.frame_shape(fr) == (r["modes"], r["nbSeq"]), n


def test_oracle_frames_decode_with_libzstd(libzstd):
    for n, (d, fr, _) in traced().items():
        assert T.zstd_decompress(fr, len(d)) == d.tobytes(), n


def test_census():
    got = reached()
    assert got >= REQUIRED, sorted(REQUIRED - got)
    for (t, m, g), why in UNREACHABLE.items():
        hit = [k for k in got if k[2] == g and t in ("*", k[0]) and m in ("*", k[1])]
        assert why and not hit, hit  # (then the argument is wrong)
    assert not any(k in REQUIRED for k in UNREACHABLE)
    long_modes = {r["modes"] for _, _, r in traced().values() if r["nbSeq"] > 336}
    assert long_modes >= MIXES, MIXES - long_modes


def test_rounds_max_is_reached_with_long_segments():
    """All 20 rounds with live steps in all 21 segments, L >= 64, in every table -- and at the
    largest L of the set for the table ordinary data does it to."""
    best = {t: max((r[t]["L"] for _, _, r in traced().values() if "rounds_max" in r[t]["tags"]), default=0) for t in M.TABLES}
    assert all(v >= 128 for v in best.values()) and best["ll"] >= 176, best


def test_exact_sequence_counts():
    tr = traced()
    for n in C.EXACT:
        assert tr["nseq_%d" % n][2]["nbSeq"] == n
    # K3's segment length on both sides of its steps, K4's whole and partial last chunks
    assert [tr["nseq_%d" % n][2]["L"] for n in (336, 337, 672, 673, 2687, 2688, 2689)] == [16, 32, 32, 48, 128, 128, 144]


def test_most_sequences_and_widest_chunk():
    """The largest sequence count the parse was driven to (L = 608 of the 640 ZH_SEQ_CAP allows)
    and the widest K4 append, as DESIGN.md records them.  No bound is asserted on the chunk; it
    is far below the sink's capacity."""
    tr = traced()
    most = max(r["nbSeq"] for _, _, r in tr.values())
    assert most == MOST_SEQUENCES and M.seglen(most) == 608 and most <= M.SEQ_CAP
    assert max(r["chunk_bits"] for _, _, r in tr.values()) == WIDEST_CHUNK_BITS < M.SW_BITS


def test_small_blocks_take_nearly_all_rounds():
    """A block of up to 22 sequences has dead segments, which hand their entry guess on unchanged
    and can never meet a stored trajectory: 18-20 rounds of one dead batch per segment (DESIGN.md:
    correct, but work nobody measured)."""
    for n in (1, 2, 16, 17, 20, 21, 22):
        r = traced()["nseq_%d" % n][2]
        assert all(18 <= r[t]["rounds"] <= 20 for t in M.TABLES), (n, r)


@pytest.mark.parametrize("broken", ("no_rounds", "entry_is_the_guess"))
def test_self_check_catches_a_scheme_without_fix_up(broken):
    """The model with its Jacobi loop deleted, or with entry(g) left at the guess, fails its own
    self-check on every case tagged rounds_max or ran_to_end: those inputs would expose a kernel
    that skipped the fix-up."""
    kw = dict(fixup=False) if broken == "no_rounds" else dict(jacobi_entry=False)
    cases = [(n, d) for n, (d, _, r) in traced().items() if any(r[t]["tags"] & {"rounds_max", "ran_to_end"} for t in M.TABLES)]
    assert len(cases) >= 10
    for n, d in cases:
        with pytest.raises(AssertionError, match="segmented scheme|final state"):
            M.trace(d, **kw)

"""GPU parity of the deep matcher alone (levels >= 5, zh_lz_deep.hip): its raw output (sequence
records, literal bytes, and on the full-search paths the per-position off << 8 | len array, read back
through the library's zh_test_lz_deep hook) equals the oracle's deep parse (oracle/zstd_oracle.c
orc_lz_parse_deep) and per-position matches (orc_deep_matches), at the edges of its search / parse
variants, chains, search, LAZY2 rule, staging and dictionary tables.  A mismatch names the first
differing sequence, literal or position.  Every case is one block of at most 64 KiB behind at most
64 KiB of prefix; the path each threshold case takes is asserted from the kernel's own path function
(zh_test_deep_path).  The inputs are built by tests/zh_deep_inputs.py and their properties checked
on the CPU by tests/test_deep_inputs.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import zh_deep_inputs as D
import zh_testlib as T

pytestmark = pytest.mark.gpu


def deep_raw(cases, depth, tables=0, nslots=None, want_off=False):
    """cases: (name, prefix, block, device byte offset).  Per item (records, literals, rle[, off])."""
    import cuda_zstd

    L = cuda_zstd.lib()
    n = len(cases)
    pre_stride = max(max(len(c[1]) for c in cases), 1)
    pre = np.zeros(n * pre_stride, np.uint8)
    blk = np.zeros(n * D.BLOCK, np.uint8)
    for i, (_, p, b, _) in enumerate(cases):
        pre[i * pre_stride:i * pre_stride + len(p)] = p
        blk[i * D.BLOCK:i * D.BLOCK + len(b)] = b
    pre_n = np.array([len(c[1]) for c in cases], np.uint32)
    blk_n = np.array([len(c[2]) for c in cases], np.uint32)
    align = np.array([c[3] for c in cases], np.uint32)
    cap, area_b = ctypes.c_uint32(), ctypes.c_uint32()
    L.zh_test_lz_sizes(ctypes.byref(cap), ctypes.byref(area_b))
    SEQ_CAP, LIT_AREA = cap.value, area_b.value
    recs = np.zeros(n * SEQ_CAP, np.uint64)
    lits = np.zeros(n * LIT_AREA, np.uint8)
    meta = np.zeros(n * 4, np.uint32)
    off = np.zeros(D.BLOCK, np.uint32) if want_off else None
    f = L.zh_test_lz_deep
    f.restype = ctypes.c_int
    vp, u = ctypes.c_void_p, ctypes.c_uint32
    f.argtypes = [vp, vp, u, vp, vp, u, vp, u, u, ctypes.c_int, u, vp, vp, vp, vp]
    rc = f(pre.ctypes.data, pre_n.ctypes.data, pre_stride, blk.ctypes.data, blk_n.ctypes.data, D.BLOCK, align.ctypes.data, n, depth, tables,
           nslots or n, recs.ctypes.data, lits.ctypes.data, meta.ctypes.data, off.ctypes.data if want_off else None)
    assert rc == 0, f"zh_test_lz_deep returned {rc}"
    out = []
    for i in range(n):
        ns, nl, rle = (int(x) for x in meta[4 * i:4 * i + 3])
        item = [recs[i * SEQ_CAP:i * SEQ_CAP + ns].copy(), lits[i * LIT_AREA:i * LIT_AREA + nl].tobytes(), rle]
        if want_off:
            item.append(off[:len(cases[i][2])].copy())
        out.append(item)
    return out


def merged(recs):
    """Deep-matcher records (walk literals before the match | length << 17 | offset << 36, no
    catch-up) -> (ll, ml, off) with a directly following same-offset match merged."""
    seqs, prev = [], 0
    for v in recs:
        v = int(v)
        cum, ln, e, off = v & 0x1FFFF, (v >> 17) & 0x7F, (v >> 24) & 0xFFF, (v >> 36) & 0x1FFFF
        assert e == 0, "the deep matcher writes no catch-up"
        ll = cum - prev
        prev = cum
        if seqs and ll == 0 and seqs[-1][2] == off:
            seqs[-1][1] += ln
        else:
            seqs.append([ll, ln, off])
    return [tuple(s) for s in seqs]


def check_item(nm, pre, blk, depth, have, need_seqs=False):
    """One item's hook result against orc_lz_parse_deep; returns the oracle's parse."""
    recs, lits, rle = have[:3]
    if D.is_rle(blk):
        assert rle == 1 and len(recs) == 0, f"{nm}: a block of one repeated byte is RLE (rle {rle}, {len(recs)} records)"
        return [], 0
    assert rle == 0, f"{nm}: RLE flag {rle} on a block that is not one repeated byte"
    want, last = D.oracle_parse(pre, blk, depth)
    assert want or not need_seqs, f"{nm}: the case must yield sequences"
    got = merged(recs)
    if got != want:
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        pos = sum(a + b for a, b, _ in want[:k])
        raise AssertionError(f"{nm} depth {depth}: sequence {k} (block position {pos}) GPU {got[k:k + 3]} oracle {want[k:k + 3]}; "
                             f"counts {len(got)} vs {len(want)}")
    exp = D.expected_literals(blk, want, last)
    if lits != exp:
        k = next((i for i, (a, b) in enumerate(zip(lits, exp)) if a != b), min(len(lits), len(exp)))
        raise AssertionError(f"{nm} depth {depth}: literal bytes differ at literal {k} of {len(lits)} (oracle {len(exp)}): "
                             f"GPU {lits[k:k + 12].hex()} oracle {exp[k:k + 12].hex()}")
    return want, last


def check_positions(nm, pre, blk, depth, off):
    """The slot's off << 8 | len per block position (a full-search path) against orc_deep_matches."""
    wl, wo = D.oracle_matches(pre, blk, depth)
    gl, go = (off & 255).astype(np.int64), (off >> 8).astype(np.int64)
    bad = np.nonzero((gl != wl) | (go != wo))[0]
    if len(bad):
        p = int(bad[0])
        raise AssertionError(f"{nm} depth {depth}: block position {p}: GPU len {gl[p]} off {go[p]}, oracle len {wl[p]} off {wo[p]} "
                             f"({len(bad)} positions differ)")


def compare(cases, depth, tables=0, nslots=None, need_seqs=False):
    got = deep_raw(cases, depth, tables, nslots)
    for have, (nm, pre, blk, _) in zip(got, cases):
        check_item(nm, pre[-D.DEEP_PRE:], blk, depth, have, need_seqs)


def compare_full(case, depth, tables=0):
    """One item alone, so the slot is still its own: parse and per-position matches.  The case must
    be on a full-search path (the demand path searches only the positions its walks reach)."""
    nm, pre, blk, _ = case
    s0 = D.deep_split(len(pre))[1] if tables else 0
    assert D.deep_path(min(len(pre), D.DEEP_PRE), len(blk), s0)[0] != D.DEMAND, f"{nm}: not a full-search path"
    have = deep_raw([case], depth, tables, want_off=True)[0]
    check_positions(nm, pre[-D.DEEP_PRE:], blk, depth, have[3])
    check_item(nm, pre[-D.DEEP_PRE:], blk, depth, have)


# ---- A. sizes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [4, 32])
def test_deep_sizes(depth):
    """Text of 1 .. 1025 bytes (below and at ZH_HASH_READ, the minimum match, one parse segment, one
    workgroup stride), the RLE probe at 1 and 2 bytes, constant bytes with only the last different."""
    compare(D.cases_sizes(), depth)


# ---- B. path thresholds -----------------------------------------------------------------------------
_threshold_cases = None


def threshold_cases():
    global _threshold_cases
    if _threshold_cases is None:
        _threshold_cases = {c[0]: c for c in D.cases_thresholds()}
    return _threshold_cases


THRESHOLDS = ("nopre_demand_last", "nopre_demand_first_off", "nopre_bytes_last", "nopre_bytes_first_off", "nopre_16384", "nopre_16385",
              "nopre_65536", "pre32k_nb32k", "pre64k_links_last", "pre64k_links_first_off", "pre64k_nb64k", "dict64k_16384", "dict64k_16385",
              "dict64k_demand_last", "dict64k_demand_first_off")


def test_deep_threshold_cases_cover_every_path():
    cases = threshold_cases()
    assert sorted(cases) == sorted(THRESHOLDS)
    assert {c[4] for c in cases.values()} == {D.DEMAND, D.LDS_BYTES, D.LDS_LINKS, D.SLOT}
    assert {c[5] for c in cases.values() if c[4] == D.DEMAND} == {16, 32, 64}


@pytest.mark.parametrize("name", THRESHOLDS)
def test_deep_path_thresholds(name):
    """Both sides of every switch of the path function (demand -> bytes and links in LDS -> links
    only -> everything from the slot; the demand path's segment lengths 16 / 32 / 64 and nseg == DT),
    without a prefix, with a prefix and no tables, and with a 64 KiB dictionary's tables.  The path
    each case takes is asserted, so a case cannot drift to the other side of a threshold."""
    nm, pre, blk, tables, path, segl = threshold_cases()[name]
    s0 = D.deep_split(len(pre))[1] if tables else 0
    assert not tables or s0 > 0
    got_path, got_segl = D.deep_path(len(pre), len(blk), s0)
    assert got_path == path, f"{nm}: path {got_path}, the case was built for {path}"
    if path == D.DEMAND:
        assert got_segl == segl, f"{nm}: segment length {got_segl}, the case was built for {segl}"
        got = deep_raw([(nm, pre, blk, 0)], 32, tables)
        check_item(nm, pre, blk, 32, got[0], need_seqs=True)
    else:
        assert D.oracle_parse(pre, blk, 32)[0], f"{nm}: the case must yield sequences"
        compare_full((nm, pre, blk, 0), 32, tables)


# ---- C. staging -------------------------------------------------------------------------------------
def test_deep_staging_alignment():
    """Device byte offsets {0, 1, 4, 15} x prefix lengths {0, 16, 17, 4104} x block sizes {4096, 4097,
    4111}: the 16-byte staging path (everything 16-byte aligned) with whole and partial last vectors,
    and the scalar path."""
    compare(D.cases_staging(), 32)


def test_deep_slot_reuse():
    """One slot (nslots = 1, items in order): a 64 KiB block, then blocks of 100, 1000 and 5000 bytes.
    The slot's bytes past n + 64 are the larger block's; only the length caps keep them out."""
    for run in D.cases_slot_reuse():
        compare(run, 32, nslots=1)


# ---- D. chains and search ---------------------------------------------------------------------------
def test_deep_periodic_chains():
    """Period-p blocks: all 64 lanes of an LDS atomic share few hashes (p = 2: every second lane),
    every match is capped at ZH_MAX_MATCH and the parse is one merged sequence to the block's end."""
    cases = D.cases_periodic()
    for depth in (4, 32):
        compare(cases, depth, need_seqs=True)
    for case in cases:
        if case[0] in ("period2_4096", "period64_20000", "period255_4096"):
            c, _ = D.census(case[1], case[2], 32)
            assert c["take64"] >= 1 and c["take_to_lim"] >= 1, case[0]


def test_deep_chain_round_boundaries():
    """lim (= n - ZH_HASH_READ) at the chain rounds' HB = 8192 boundaries and 256 +- 1 positions past a
    round start (the inner step): lanes at and past lim go to the junk slot."""
    compare(D.cases_lims(), 32, need_seqs=True)


@pytest.mark.parametrize("d", D.D_DEPTHS)
def test_deep_depth_cutoff(d):
    """key + tail, k lone keys, key + tail: at depth d the 45-byte match is candidate k + 1, taken
    with k = d - 1 and not with k = d."""
    compare(D.cases_decoys(d), d, need_seqs=True)  # (the inputs discriminate: tests/test_deep_inputs.py)


def test_deep_offset_bound():
    """Offsets 65536 (rejected), 65535 and 65534 (accepted) through a u16 link distance, and a near
    candidate in range whose next link is out of range; without the tables (links in LDS from the
    block's own chains) and with them (the candidate's next link comes from the dictionary's)."""
    cases = D.cases_offset_bound()
    for depth in (4, 32):
        for tables in (0, 1):
            for case in cases:
                if tables:  # (a short block behind the tables is on the demand path: the parse alone)
                    assert D.deep_path(D.DEEP_PRE, len(case[2]), D.deep_split(D.DEEP_PRE)[1])[0] == D.DEMAND
                    compare([case], depth, tables=1)
                else:
                    compare_full(case, depth)


# ---- E. LAZY2 margins -------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,seed", D.E_INPUTS)
def test_deep_lazy2_margins(depth, seed):
    """16 KiB of text whose serial parse decides at each exact margin of the LAZY2 rule (g1 == g0 + 4
    taken, g0 + 5 deferred; g2 == g0 + 7 taken, g0 + 8 deferred) at least once -- the census, asserted
    first -- on the demand path (the memo form of the rule) and, behind a prefix without tables, on
    a full-search path (the take-mask form)."""
    for with_prefix in (False, True):
        nm, pre, blk, _ = case = D.cases_lazy(depth, seed, with_prefix)
        c, parse = D.census(pre, blk, depth)
        assert parse == D.oracle_parse(pre, blk, depth)[0]
        for k in D.E_FLOORS:
            assert c[k] >= 1, f"{nm}: no parse step at margin {k}: {c}"
        if with_prefix:
            compare_full(case, depth)
        else:
            assert D.deep_path(0, len(blk))[0] == D.DEMAND
            compare([case], depth)


# ---- F. dictionary tables ---------------------------------------------------------------------------
def test_deep_dict_tables():
    """Dictionary content of 71 (no tables), 72, 75, 76, 1000, 1021, 65536 and 70000 bytes and a JSON
    block that repeats content bytes from below the split, from [split, pre) and across the content /
    block boundary: with the tables, without them and the oracle all give the same parse."""
    cases = D.cases_dict()
    assert [D.deep_split(len(c[1]))[0] > 0 for c in cases] == [False] + [True] * (len(cases) - 1)
    for depth in (4, 32):
        with_t = deep_raw([(nm, content, blk, 0) for nm, content, blk in cases], depth, tables=1)
        without = deep_raw([(nm, content[-D.DEEP_PRE:], blk, 0) for nm, content, blk in cases], depth, tables=0)
        for (nm, content, blk), a, b in zip(cases, with_t, without):
            want, _ = check_item(nm + " (tables)", content[-D.DEEP_PRE:], blk, depth, a, need_seqs=True)
            check_item(nm + " (no tables)", content[-D.DEEP_PRE:], blk, depth, b, need_seqs=True)
            assert merged(a[0]) == merged(b[0]) == want and a[1] == b[1], nm


# ---- G. the forced fix-up variant -------------------------------------------------------------------
def test_forced_fixup_variant(tmp_path):
    """deep_chains' out-of-order fix-up never runs on this hardware.  The -DZH_DEEP_FORCE_FIXUP=1
    build takes it at every chain step: the chain inputs (D) and the dictionary inputs (F) through the
    hook and a handful of them as level-9 frames, in a child process on that library
    (CUDA_ZSTD_HIP_LIB), must give the oracle's parses and frames."""
    import deep_fixup_data as W

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(root, "custom-nvcomp-with-zstd_amd", W.LIB_NAME)
    assert os.path.exists(so), "build() makes the forced fix-up variant"
    out = tmp_path / "ff.npz"
    subprocess.run([sys.executable, os.path.join(root, "tests", "deep_fixup_worker.py"), str(out)], env=dict(os.environ, CUDA_ZSTD_HIP_LIB=so),
                   check=True, timeout=300)
    r = np.load(out)
    for k, (nm, pre, blk, tables, depth) in enumerate(W.hook_cases()):
        have = [r[f"recs{k}"], r[f"lits{k}"].tobytes(), int(r[f"rle{k}"][0])]
        check_item(f"fix-up build, {nm}" + (" (tables)" if tables else ""), pre[-D.DEEP_PRE:], blk, depth, have, need_seqs=True)
    frames = W.frame_inputs()
    sizes = r["frame_sizes"].tolist()
    blob = r["frames"].tobytes()
    assert len(sizes) == len(frames)
    pos = 0
    for (nm, d), sz in zip(frames, sizes):
        assert blob[pos:pos + sz] == T.oracle_frame(d, level=9), f"fix-up build, level-9 frame of {nm} differs from the oracle's"
        pos += sz

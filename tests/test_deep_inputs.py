"""CPU side of tests/test_gpu_deep.py: the properties its inputs must have for the GPU comparison
to mean anything, from the oracle alone (no device): the depth decoys discriminate, the offset-bound
cases give 0, 1 and 1 sequences, the LAZY2 census floors hold, the periodic inputs are one capped,
merged sequence; and -- when the HIP library loads without a device -- the path function's
thresholds are bracketed by the threshold cases."""
import pytest

import zh_deep_inputs as D


def test_orc_deep_matches_is_the_parse_input():
    """orc_lz_parse_deep parses orc_deep_matches: the census's serial walk over the exported matches
    reproduces the oracle's own parse, with and without a prefix."""
    for depth, seed in D.E_INPUTS:
        for with_prefix in (False, True):
            _, pre, blk, _ = D.cases_lazy(depth, seed, with_prefix)
            assert D.census(pre, blk, depth)[1] == D.oracle_parse(pre, blk, depth)[0]


@pytest.mark.parametrize("d", D.D_DEPTHS)
def test_decoys_discriminate(d):
    """With k = d - 1 lone keys the 45-byte match is candidate d: found at depth d, not at d - 1;
    with k = d it is candidate d + 1: not found at depth d, found at d + 1.  The parses differ."""
    for k, found in ((d - 1, True), (d, False)):
        blk = D.decoy(k)
        p = D.decoy_pos(k)  # the last key
        for depth, want in ((d, found), (d - 1 if found else d + 1, not found)):
            ln, off = D.oracle_matches(D.EMPTY, blk, depth)
            assert (ln[p] == 45 and off[p] == 45 + D.DECOY * k) == want, (k, depth, ln[p], off[p])
            if not want:
                assert ln[p] == 5 and off[p] == D.DECOY, (k, depth, ln[p], off[p])
        assert D.oracle_parse(D.EMPTY, blk, d)[0] != D.oracle_parse(D.EMPTY, blk, d - 1 if found else d + 1)[0], k


def test_offset_bound_inputs():
    cases = {c[0]: c for c in D.cases_offset_bound()}
    for nm, nseq in (("offset65536", 0), ("offset65535", 1), ("offset65534", 1)):
        seqs, _ = D.oracle_parse(cases[nm][1], cases[nm][2], 32)
        assert len(seqs) == nseq, (nm, seqs)
        if nseq:
            assert seqs[0] == (0, 200, int(nm[6:])), (nm, seqs)
    # the near candidate alone (10 bytes) when the far one is 65536 away, the far one (20) at 65535
    # (depth 32: the random prefix puts a few colliding positions on the chain between the two)
    assert D.oracle_parse(*cases["near_then_65536"][1:3], 32)[0] == [(100, 10, 25636)]
    ln, off = D.oracle_matches(*cases["near_then_65535"][1:3], 32)
    assert (ln[99], off[99]) == (20, 65535)


def test_lazy2_census_floors():
    for depth, seed in D.E_INPUTS:
        for with_prefix in (False, True):
            nm, pre, blk, _ = D.cases_lazy(depth, seed, with_prefix)
            c, _ = D.census(pre, blk, depth)
            for k in D.E_FLOORS:
                assert c[k] >= 1, f"{nm}: no parse step at margin {k}: {c}"


def test_periodic_inputs_are_one_capped_sequence():
    for nm, pre, blk, _ in D.cases_periodic():
        p = int(nm[6:].split("_")[0])
        for depth in (4, 32):
            c, seqs = D.census(pre, blk, depth)
            assert len(seqs) == 1 and seqs[0][0] == p and seqs[0][2] == p, (nm, seqs)
            assert c["take64"] >= 1 and c["take_to_lim"] == 1, (nm, c)


def test_dict_inputs_yield_sequences():
    for nm, content, blk in D.cases_dict():
        assert D.oracle_parse(content[-D.DEEP_PRE:], blk, 32)[0], nm


def test_path_thresholds_are_bracketed():
    """Every path is taken by a case, every switch of the path function has the case on each side of
    it, and the three demand segment lengths occur."""
    try:
        D.deep_lib()
    except (OSError, ImportError) as e:
        pytest.skip(f"the HIP library does not load here: {e}")
    cases = {c[0]: c for c in D.cases_thresholds()}
    for nm, pre, blk, tables, path, segl in cases.values():
        s0 = D.deep_split(len(pre))[1] if tables else 0
        got = D.deep_path(len(pre), len(blk), s0)
        assert got[0] == path and (path != D.DEMAND or got[1] == segl), (nm, got)
    for last, first in (("nopre_demand_last", "nopre_demand_first_off"), ("nopre_bytes_last", "nopre_bytes_first_off"),
                        ("pre64k_links_last", "pre64k_links_first_off"), ("dict64k_demand_last", "dict64k_demand_first_off"),
                        ("nopre_16384", "nopre_16385"), ("dict64k_16384", "dict64k_16385")):
        a, b = cases[last], cases[first]
        assert len(b[2]) == len(a[2]) + 1 and len(a[1]) == len(b[1]) and (a[4], a[5]) != (b[4], b[5]), (last, first)
    assert {c[4] for c in cases.values()} == {D.DEMAND, D.LDS_BYTES, D.LDS_LINKS, D.SLOT}
    assert {c[5] for c in cases.values() if c[4] == D.DEMAND} == {16, 32, 64}

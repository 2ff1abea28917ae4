"""CPU census of the table-builder cases (tests/zh_table_cases.py) and of the end-to-end inputs
(tests/zh_table_inputs.py): every required branch tag is met by a directed case, as the oracle's
branch trace shows; a tag argued unreachable is met by no case of any set; two builds give the
same cases; the oracle equals libzstd 1.4.9's recorded results on the directed cases
(tests/golden/fse_tables_directed.json, huf_tables_directed.json), value for value; and the trace
shows which whole input takes FSE_normalizeM2 in which sequence table at which level, so the GPU
run of tests/test_gpu_tables.py is known to execute the device's m2."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import zh_table_cases as C
import zh_table_inputs as I
import zh_testlib as T


@pytest.fixture(scope="module")
def sets():
    """{builder: {set: (cases, tags met, results)}}"""
    out = {}
    for b, parts, orc, tagger in (("fse", (("directed", C.fse_directed), ("grid", C.fse_grid), ("random", C.fse_random)), C.fse_oracle, C.fse_tags),
                                  ("huf", (("directed", C.huf_directed), ("grid", C.huf_grid), ("random", C.huf_random)), C.huf_oracle, C.huf_tags)):
        out[b] = {}
        for name, make in parts:
            cases = make()
            hit, res = C.census(cases, orc, tagger)
            out[b][name] = (cases, hit, res)
    return out


def test_trace_sites_are_named():
    names = C.trace_names()
    assert len(names) == len(set(names)) and "N_M2" in names and "H_REPAY_NOSYM" in names
    C.trace_reset()
    assert C.trace_read() == {}
    sites = {s for yes, no in list(C.FSE_TRACE_TAGS.values()) + list(C.HUF_TRACE_TAGS.values()) for s in yes + no}
    assert sites <= set(names), sites - set(names)


@pytest.mark.parametrize("builder,required", (("fse", C.FSE_REQUIRED), ("huf", C.HUF_REQUIRED)))
def test_census_directed_cases_meet_every_tag(sets, builder, required):
    cases, hit, _ = sets[builder]["directed"]
    print(f"{builder}: {len(cases)} directed cases")
    for t in required:
        print(f"  {t:36s} {len(hit.get(t, [])):4d}  {hit.get(t, ['-'])[0]}")
    missing = [t for t in required if t not in hit and t not in C.UNREACHED]
    assert not missing, missing
    assert len(set(c.name for c in cases)) == len(cases)


def test_unreached_rule(sets):
    """UNREACHED holds only required tags that carry a reason, none of those shown reachable, and
    no case of any set meets one (error returns included: every case is inside the domain)."""
    req = set(C.FSE_REQUIRED) | set(C.HUF_REQUIRED)
    assert set(C.UNREACHED) <= req
    assert not set(C.UNREACHED) & set(C.NEVER_UNREACHED)
    assert set(C.NEVER_UNREACHED) <= req
    assert all(len(why) > 60 for why in C.UNREACHED.values())
    for b in sets:
        for name, (cases, hit, _) in sets[b].items():
            met = set(hit) & (set(C.UNREACHED) | {"normalize_error", "ncount_error"})
            assert not met, (b, name, {t: hit[t][:3] for t in met})


def test_sets_are_deterministic_and_sized(sets):
    for b, parts in (("fse", (("directed", C.fse_directed), ("grid", C.fse_grid), ("random", C.fse_random))),
                     ("huf", (("directed", C.huf_directed), ("grid", C.huf_grid), ("random", C.huf_random)))):
        for name, make in parts:
            again = make()
            cases = sets[b][name][0]
            assert [c.name for c in again] == [c.name for c in cases]
            assert all((x.count == y.count).all() and x[2:] == y[2:] for x, y in zip(again, cases))
    n = {b: {k: len(v[0]) for k, v in sets[b].items()} for b in sets}
    print(n)
    assert n["fse"]["random"] == 1000 and n["huf"]["random"] == 1000
    assert 1000 <= n["fse"]["directed"] + n["fse"]["grid"] <= 6000 and 1000 <= n["huf"]["directed"] + n["huf"]["grid"] <= 6000


def test_cases_are_inside_the_builders_domain(sets):
    for name, (cases, _, res) in sets["fse"].items():
        for c, r in zip(cases, res):
            assert C.fse_valid(c) and c.maxsv in C.FSE_MAXSV + C.FSE_MAXSV_EXTRA and c.total == int(c.count.sum()), c.name
            assert r.ret == c.tablelog and len(r.ncount) > 0, c.name
    for name, (cases, _, res) in sets["huf"].items():
        for c, r in zip(cases, res):
            assert C.huf_valid(c) and 0 < r.hufflog <= c.maxbits, c.name


def test_forced_and_optimal_table_logs_both_present(sets):
    cases = sets["fse"]["directed"][0]
    opt = [c for c in cases if c.tablelog == C.optimal_table_log(C.FSE_MAXLOG.get(c.maxsv, 9), c.total, c.maxsv, 2)]
    assert opt and len(opt) < len(cases)
    assert {c.tablelog for c in cases} == {5, 6, 7, 8, 9} and {c.low for c in cases} == {0, 1}
    assert {c.maxsv for c in cases} >= set(C.FSE_MAXSV)
    o = T.oracle()
    for c in cases[:50]:
        assert o.orc_fse_optimal_table_log(ctypes.c_uint32(9), ctypes.c_size_t(c.total), ctypes.c_uint32(c.maxsv)) == \
            C.optimal_table_log(9, c.total, c.maxsv, 2)


def test_deepest_tree_is_the_deepest(sets):
    """gen_deepest's argument, checked: the chain has code length DEEPEST, and one more leaf by the
    slowest-growth rule no longer fits a block's literals."""
    c = C.gen_deepest()
    assert sum(c) <= C.LIT_MAX < sum(c) + max(c[-1], sum(c[:-1]))
    r = C.huf_oracle(C._huf_case("deepest", c, 12))
    assert r.trace["H_LARGEST_BITS"] == C.DEEPEST == len(c) - 1


def _golden(name):
    with open(os.path.join(T.GOLDEN, name)) as f:
        g = json.load(f)
    assert g["libzstd_version"] == 10409
    return g["cases"]


def test_oracle_equals_libzstd_on_directed_fse_cases(sets):
    cases, _, res = sets["fse"]["directed"]
    gold = {g["name"]: g for g in _golden("fse_tables_directed.json")}
    assert set(gold) == {c.name for c in cases}, "every directed case is one libzstd accepts: regenerate with make_golden.py tables"
    for c, r in zip(cases, res):
        g = gold[c.name]
        assert g["counts"] == c.count[:c.maxsv + 1].tolist() and (g["maxsv"], g["tablelog"], g["lowprob"]) == (c.maxsv, c.tablelog, c.low), c.name
        assert r.norm.tolist() == g["norm"], c.name
        assert r.ncount.hex() == g["ncount"], c.name


def test_oracle_equals_libzstd_on_directed_huf_cases(sets):
    cases, _, res = sets["huf"]["directed"]
    gold = {g["name"]: g for g in _golden("huf_tables_directed.json")}
    assert set(gold) == {c.name for c in cases}
    for c, r in zip(cases, res):
        g = gold[c.name]
        assert g["counts_sha256"] == hashlib.sha256(c.count.astype("<u4").tobytes()).hexdigest(), c.name
        assert (g["maxsv"], g["maxbits"]) == (c.maxsv, c.maxbits), c.name
        assert r.hufflog == g["huflog"], c.name
        assert r.nbits[:c.maxsv + 1].tobytes().hex() == g["nbits"], c.name
        assert r.val[:c.maxsv + 1].astype("<u2").tobytes().hex() == g["val"], c.name
        assert (r.header.hex() if r.header else None) == g["header"], c.name


def test_libzstd_agrees_now(libzstd):
    """Where libzstd 1.4.9 is present, its FSE_normalizeCount agrees with the oracle on the grid
    and random FSE cases as well (the fixtures hold the directed ones only)."""
    z = libzstd
    if int(z.ZSTD_versionNumber()) != 10409:
        pytest.skip("fixtures are libzstd 1.4.9's")
    z.FSE_normalizeCount.restype = ctypes.c_size_t
    for c in C.fse_grid() + C.fse_random():
        norm = np.zeros(256, np.int16)
        cnt = np.ascontiguousarray(c.count, np.uint32)
        r = z.FSE_normalizeCount(norm.ctypes.data_as(T.vp), ctypes.c_uint(c.tablelog), cnt.ctypes.data_as(T.vp), ctypes.c_size_t(c.total),
                                 ctypes.c_uint(c.maxsv), ctypes.c_uint(c.low))
        assert r == c.tablelog, c.name
        assert norm[:c.maxsv + 1].tolist() == C.fse_oracle(c).norm.tolist(), c.name


def test_hooks_refuse_arguments_outside_the_domain():
    """The GPU hooks check their arguments on the host before any device call: nothing is launched for a table log below FSE_minTableLog, a single used symbol, a total that
    is not the counts' sum, or a code length limit too small for the alphabet."""
    import cuda_zstd as gpu

    one = np.zeros((1, 64), np.uint32)
    one[0, :40] = 1
    for par in ([39, 40, 5, 0], [39, 41, 6, 0], [64, 40, 6, 0], [39, 40, 10, 0]):
        with pytest.raises(RuntimeError, match="returned 2"):
            gpu._test_fse_table(one, np.array([par], np.uint32))
    solo = np.zeros((1, 64), np.uint32)
    solo[0, 3] = 40
    with pytest.raises(RuntimeError, match="returned 2"):
        gpu._test_fse_table(solo, np.array([[3, 40, 6, 0]], np.uint32))
    h = np.zeros((1, 256), np.uint32)
    h[0, :40] = 1
    for par in ([39, 5], [39, 13], [256, 11]):
        with pytest.raises(RuntimeError, match="returned 2"):
            gpu._test_huf_table(h, np.array([par], np.uint32))
    h[0, 1:] = 0
    with pytest.raises(RuntimeError, match="returned 2"):
        gpu._test_huf_table(h, np.array([[39, 11]], np.uint32))


def test_inputs_reach_m2():
    """Which table of which input takes m2 at which level, from the trace of the oracle's own frame;
    LL and ML at level 3 (K2's fast-matcher path) and OF at 5 and 9 are among them."""
    names = [n for n, _ in I.cases()]
    assert set(I.REACH) == set(names) and len(set(names)) == len(names)
    seen = set()
    for name, d in I.cases():
        assert 0 < len(d) <= 65536
        for lv in I.LEVELS:
            C.trace_reset()
            T.oracle_frame(d, level=lv)
            tr = C.trace_read()
            got = " ".join(t for t, s in (("LL", "SEQ_M2_LL"), ("OF", "SEQ_M2_OF"), ("ML", "SEQ_M2_ML")) if tr.get(s))
            assert got == I.REACH[name].get(lv, ""), (name, lv, got)
            seen |= {(t, lv) for t in got.split()}
    assert {("LL", 3), ("ML", 3), ("OF", 5), ("OF", 9), ("LL", 1), ("ML", 1), ("LL", 9), ("ML", 9)} <= seen
    assert not {("OF", 1), ("OF", 2), ("OF", 3)} & seen and "OF at levels 1-3" in I.UNREACHED

"""Directed inputs for K2's table builders (fse_normalize_wave / fse_normalize_m2,
fse_write_ncount_wave, fse_build_ctable_par, huf_build_ctable_par / huf_set_max_height,
huf_write_ctable_wave; csrc/zh_entropy.hip), the oracle's results for them, and the branch tags
each one meets.  A tag is read from the oracle's branch trace (orc_trace_*, oracle/zstd_oracle.c)
or from the oracle's result; the cases were found by searching the generators below with that trace
and are rebuilt from (generator, arguments, seed), so two builds give the same cases.

Three sets per builder:
  directed  one or a few witnesses per tag; pinned to libzstd 1.4.9 by tests/golden/
            fse_tables_directed.json / huf_tables_directed.json (tests/golden/make_golden.py tables)
  grid      every generator at every shape (maxSV x tableLog x useLowProbCount / used symbols x maxNbBits)
  random    seeded draws of the same generators and shapes
tests/test_table_cases.py holds the census, tests/test_gpu_tables.py runs all of them on the GPU."""
import ctypes
import functools
from collections import namedtuple

import numpy as np

import zh_testlib as T

vp = ctypes.c_void_p
FseCase = namedtuple("FseCase", "name count maxsv total tablelog low")      # count: uint32[64]
HufCase = namedtuple("HufCase", "name count maxsv maxbits")                 # count: uint32[256]

FSE_MAXSV = (1, 2, 12, 28, 31, 35, 52, 63)
# m2's "all distributed" exit needs every symbol of the alphabet used and at least T / 1.5 of them
# while total < T: of all alphabets only 43 symbols under a 64-cell table do it (maxSV 42, a
# match-length or literal-length alphabet whose last used code is 42)
FSE_MAXSV_EXTRA = (42,)
FSE_MAXLOG = {12: 6, 31: 8}          # the weights' and the offsets' table; every other shape: 9 (LL, ML)
LIT_MAX = 1 << 17                    # literals (and sequences) of one block


# ---------------------------------------------------------------- the oracle, traced
def _oracle():
    o = T.oracle()
    o.orc_trace_read.restype = ctypes.c_uint32
    o.orc_trace_name.restype = ctypes.c_char_p
    o.orc_fse_build_ctable.restype = ctypes.c_int
    return o


@functools.lru_cache(None)
def trace_names():
    o = _oracle()
    n = o.orc_trace_read(None, 0)
    return tuple(o.orc_trace_name(ctypes.c_uint32(i)).decode() for i in range(n))


def trace_reset():
    _oracle().orc_trace_reset()


def trace_read():
    """{site: count} of the sites met since trace_reset() on this thread."""
    names = trace_names()
    a = np.zeros(len(names), np.uint32)
    _oracle().orc_trace_read(a.ctypes.data_as(vp), ctypes.c_uint32(len(a)))
    return {n: int(v) for n, v in zip(names, a) if v}


def highbit(v):
    return int(v).bit_length() - 1


def min_table_log(total, maxsv):
    return min(highbit(total) + 1, highbit(maxsv) + 2)


def optimal_table_log(max_log, total, maxsv, minus):
    """FSE_optimalTableLog_internal (minus 2: FSE tables, 1: HUF_optimalTableLog)."""
    return min(12, max(5, min_table_log(total, maxsv), min(max_log, highbit(total - 1) - minus)))


FseResult = namedtuple("FseResult", "ret norm ncount st sym trace")  # st / sym None unless ncount


def fse_oracle(c):
    """orc_fse_normalize, orc_fse_write_ncount and orc_fse_build_ctable on one case.  ret: the
    normalisation's return (-1 error); ncount b"" if it failed; sym: (dNb, dFS) rows."""
    o = _oracle()
    cnt = np.ascontiguousarray(c.count, np.uint32)
    norm = np.zeros(64, np.int16)
    trace_reset()
    ret = o.orc_fse_normalize(norm.ctypes.data_as(vp), ctypes.c_uint32(c.tablelog), cnt.ctypes.data_as(vp), ctypes.c_size_t(c.total),
                              ctypes.c_uint32(c.maxsv), ctypes.c_int(c.low))
    nc, st, sym = b"", None, None
    if ret > 0:
        buf = np.zeros(512, np.uint8)
        h = o.orc_fse_write_ncount(buf.ctypes.data_as(vp), ctypes.c_size_t(512), norm.ctypes.data_as(vp), ctypes.c_uint32(c.maxsv),
                                   ctypes.c_uint32(c.tablelog))
        nc = buf[:h].tobytes()
        if h:
            ct = np.zeros(4 + 2 * 4096 + 8 * 256, np.uint8)  # fse_ctable_t {u32 tableLog; u16 stateTable[4096]; {s32 dFS; u32 dNb} sym[256]}
            r = o.orc_fse_build_ctable(ct.ctypes.data_as(vp), norm.ctypes.data_as(vp), ctypes.c_uint32(c.maxsv), ctypes.c_uint32(c.tablelog))
            assert r == 0, c.name
            st = ct[4:4 + 2 * 4096].view(np.uint16)[:1 << c.tablelog].copy()
            sy = ct[4 + 2 * 4096:].view(np.uint32).reshape(256, 2)[:c.maxsv + 1]
            sym = np.stack([sy[:, 1], sy[:, 0]], 1).copy()
    return FseResult(ret, norm[:c.maxsv + 1].copy(), nc, st, sym, trace_read())


HufResult = namedtuple("HufResult", "hufflog nbits val header trace wtrace")


def huf_oracle(c):
    """orc_huf_build_ctable and orc_huf_write_ctable on one case (header b"" where none can be
    written); trace: the build's sites, wtrace: the header's (the weights' own normalisation)."""
    o = _oracle()
    cnt = np.ascontiguousarray(c.count, np.uint32)
    tree = np.zeros(256 * 2, np.uint16)  # huf_celt_t {u16 val; u8 nbBits; pad}
    trace_reset()
    hl = int(o.orc_huf_build_ctable(tree.ctypes.data_as(vp), cnt.ctypes.data_as(vp), ctypes.c_uint32(c.maxsv), ctypes.c_uint32(c.maxbits)))
    tr = trace_read()
    hdr, wtr = b"", {}
    if hl:
        buf = np.zeros(512, np.uint8)
        trace_reset()
        h = o.orc_huf_write_ctable(buf.ctypes.data_as(vp), ctypes.c_size_t(512), tree.ctypes.data_as(vp), ctypes.c_uint32(c.maxsv), ctypes.c_uint32(hl))
        wtr = trace_read()
        hdr = buf[:h].tobytes()
    e = tree.reshape(256, 2)
    return HufResult(hl, (e[:, 1] & 0xFF).astype(np.uint8), e[:, 0].copy(), hdr, tr, wtr)


# ---------------------------------------------------------------- tags
ZRUNS = (1, 2, 3, 5, 6, 23, 24, 25, 27, 48, 51)
FSE_TRACE_TAGS = {  # tag: (sites all met, sites none met)
    "m2_trigger_exact": (("N_M2", "N_M2_EXACT"), ()),
    "largest_absorbs_one_less": (("N_LARGEST_ONE_LESS",), ("N_M2",)),
    "still_positive": (("N_STILL_POS",), ()),
    "tie_for_largest": (("N_TIE_LARGEST",), ("N_M2",)),
    "largest_at_lane0": (("N_LARGEST_AT0",), ("N_M2",)),
    "largest_at_lane_maxsv": (("N_LARGEST_AT_MAXSV",), ("N_M2",)),
    "m2_rstep": (("M2_RSTEP",), ()),
    "m2_all_distributed": (("M2_ALLDIST",), ()),
    "m2_all_distributed_tie": (("M2_ALLDIST_TIE",), ()),
    "m2_second_low_one_pass": (("M2_SECOND_PASS_TAKEN",), ()),
    "m2_total0_round_robin": (("M2_TOTAL0",), ()),
    "m2_total0_wrap": (("M2_TOTAL0_WRAP",), ()),
    "m2_to_distribute0": (("M2_TODIST0",), ()),
    "m2_weight_below1": (("M2_WEIGHT0",), ()),
    "count_eq_low_threshold": (("N_EQ_LOWTHR",), ()),
    "count_eq_low_threshold_plus1": (("N_EQ_LOWTHR1",), ()),
    "ncount_run_to_end": (("NC_RUN_END",), ()),
    "ncount_flush_after_run": (("NC_FLUSH_RUN",), ()),
    "ncount_flush_after_count": (("NC_FLUSH_COUNT",), ()),
    "ncount_count_ge_threshold": (("NC_GE_THRESHOLD",), ()),
    "ncount_short_code": (("NC_SHORT",), ()),
    "ncount_remaining1_early": (("NC_REM1_EARLY",), ()),
}
for _p in range(8):
    FSE_TRACE_TAGS[f"rtb{_p}_up"] = ((f"N_RTB_UP{_p or ''}",), ())
    FSE_TRACE_TAGS[f"rtb{_p}_down"] = ((f"N_RTB_DOWN{_p or ''}",), ())


def zero_runs(norm):
    """Lengths of the maximal runs of zero probabilities, and whether the last reaches the end."""
    runs, n = [], 0
    for v in norm:
        if v == 0:
            n += 1
        elif n:
            runs.append(n)
            n = 0
    return runs, n


def fse_tags(c, r):
    tags = set()
    for tag, (yes, no) in FSE_TRACE_TAGS.items():
        if all(s in r.trace for s in yes) and not any(s in r.trace for s in no):
            tags.add(tag)
    if r.ret < 0:
        tags.add("normalize_error")
        return tags
    if not r.ncount:
        tags.add("ncount_error")
        return tags
    norm = r.norm.tolist()
    used = sum(1 for v in norm if v)
    nlow = sum(1 for v in norm if v == -1)
    tags.add("nlow_0" if nlow == 0 else "nlow_1" if nlow == 1 else "nlow_several")
    if used >= 3 and nlow == used - 1:
        tags.add("nlow_all_but_one")
    first, last = next(i for i, v in enumerate(norm) if v), max(i for i, v in enumerate(norm) if v)
    if any(v == 0 for v in norm[first:last]):
        tags.add("ctable_zero_between_used")
    if c.tablelog in (5, 9):
        tags.add(f"states_{1 << c.tablelog}")
    runs, tail = zero_runs(norm)
    for n in runs:
        if n in ZRUNS:
            tags.add(f"ncount_zero_run_{n}")
    if tail:
        tags.add("norm_zero_tail")  # the run to the end of the alphabet (never written: remaining is 1)
    return tags


HUF_USED = (2, 3, 32, 33, 64, 65, 128, 129, 255, 256)
DEEPEST = 24  # code length of the deepest tree <= LIT_MAX literals give: see gen_deepest
HUF_TRACE_TAGS = {
    "limit_repay_no_rank1": (("H_REPAY_NOSYM",), ()),
    "limit_repay_rank1": (("H_REPAY_SYM",), ()),
    "limit_ranklast_reaches_0": (("H_RANKLAST0",), ()),
    "limit_lowpos_break": (("H_LOWPOS_BREAK",), ()),
    "limit_highpos_continue": (("H_HIGHPOS_CONT",), ()),
    "limit_walk_up_empty_rank": (("H_WALKUP",), ()),
    "limit_count_break": (("H_COUNT_BREAK",), ()),
    "limit_fill_lower_rank": (("H_FILL_LOWER",), ()),
    "limit_rank_emptied": (("H_RANK_EMPTIED",), ()),
    "merge_tie_leaf_node": (("H_TIE_LEAF_NODE",), ()),
}


def huf_tags(c, r):
    tags = set()
    for tag, (yes, no) in HUF_TRACE_TAGS.items():
        if all(s in r.trace for s in yes) and not any(s in r.trace for s in no):
            tags.add(tag)
    cnt = c.count[:c.maxsv + 1]
    used = int((cnt != 0).sum())
    if used in HUF_USED:
        tags.add(f"used_{used}")
    nz = cnt[cnt != 0]
    if used >= 4 and (nz == nz[0]).all():
        tags.add("all_counts_equal")
    elif used >= 8 and len(np.unique(nz)) <= used // 4:
        tags.add("blocks_of_equal_counts")
    if used < c.maxsv + 1 and (cnt[:c.maxsv] == 0).any():
        tags.add("hole_below_maxsv")
    depth = r.trace.get("H_LARGEST_BITS", 0)
    fib = c.name[:3] == "fib" and c.name[3:4].isdigit()  # the hand-made pure Fibonacci counts
    if fib and depth == 11 and c.maxbits == 11:
        tags.add("fibonacci_depth_11_no_limit")
    if fib and depth == 12 and c.maxbits == 11:
        tags.add("fibonacci_depth_12_limited")
    if depth >= DEEPEST:
        tags.add("deepest_tree")
    if c.name.startswith("pow2"):
        tags.add("powers_of_two")
    if "H_LIMIT" in r.trace:
        tags.add("depth_limited")
    tags.add("maxbits_11" if c.maxbits == 11 else "maxbits_k2" if c.maxbits == optimal_table_log(11, int(cnt.sum()), c.maxsv, 1) else "maxbits_forced")
    if c.maxbits == optimal_table_log(11, int(cnt.sum()), c.maxsv, 1) and c.maxbits != 11:
        tags.add("maxbits_k2_below_11")
    if not r.header:
        tags.add("header_none")
    elif r.header[0] >= 128:
        tags.add("header_direct")
    else:
        tags.add("header_fse")
    if "N_M2" in r.wtrace:
        tags.add("weights_m2")
    return tags


FSE_REQUIRED = (
    "m2_trigger_exact", "largest_absorbs_one_less", "still_positive", "tie_for_largest", "largest_at_lane0", "largest_at_lane_maxsv",
    "m2_rstep", "m2_all_distributed", "m2_all_distributed_tie", "m2_second_low_one_pass", "m2_total0_round_robin", "m2_total0_wrap",
    "m2_to_distribute0", "m2_weight_below1", "count_eq_low_threshold", "count_eq_low_threshold_plus1",
    *[f"rtb{p}_{d}" for p in range(8) for d in ("up", "down")],
    "nlow_0", "nlow_1", "nlow_several", "nlow_all_but_one", "ctable_zero_between_used", "states_32", "states_512",
    *[f"ncount_zero_run_{n}" for n in ZRUNS], "norm_zero_tail", "ncount_run_to_end", "ncount_flush_after_run", "ncount_flush_after_count",
    "ncount_count_ge_threshold", "ncount_short_code", "ncount_remaining1_early")
HUF_REQUIRED = (
    *[f"used_{n}" for n in HUF_USED], "all_counts_equal", "blocks_of_equal_counts", "hole_below_maxsv", "fibonacci_depth_11_no_limit",
    "fibonacci_depth_12_limited", "deepest_tree", "powers_of_two", "limit_repay_no_rank1", "limit_repay_rank1", "limit_ranklast_reaches_0",
    "limit_lowpos_break", "limit_highpos_continue", "limit_walk_up_empty_rank", "maxbits_11", "maxbits_k2_below_11", "maxbits_forced",
    "header_direct", "header_fse", "weights_m2")
# May never be argued away (they are shown reachable): the census rejects them in UNREACHED.
NEVER_UNREACHED = ("m2_trigger_exact", "largest_absorbs_one_less", "still_positive", "tie_for_largest", "largest_at_lane0",
                   "largest_at_lane_maxsv", "m2_rstep", "m2_all_distributed", "m2_all_distributed_tie", "fibonacci_depth_11_no_limit",
                   "fibonacci_depth_12_limited", "deepest_tree", "powers_of_two", "limit_repay_no_rank1", "limit_repay_rank1",
                   "limit_ranklast_reaches_0", "limit_lowpos_break", "limit_highpos_continue", "limit_walk_up_empty_rank")

# Tags no valid input meets, each with the argument; the census fails if any case ever meets one.
# "Valid" is FSE_normalizeCount's own argument check, which K2's fse_optimal_table_log always
# satisfies: tableLog >= FSE_minTableLog = min(highbit(total) + 1, highbit(maxSV) + 2), so the table
# size T = 2^tableLog exceeds min(total, maxSV + 1), hence the number of used symbols.  (Besides
# the arguments: 118,208 valid random cases over every maxSV 1-63, tableLog 5-9 and four generators
# of small, sparse and mixed counts met none of them.)
UNREACHED = {
    "m2_to_distribute0": "toDistribute = T - distributed, and distributed counts used symbols only: at most min(total, maxSV + 1) < T.",
    "m2_weight_below1": "A symbol left for the rStep loop has count > lowOne >= total / toDistribute (the second pass raises lowOne to "
                        "1.5 total / toDistribute when that fails), so count * toDistribute >= total + 1 and count * rStep >= "
                        "2^vStepLog (1 + 1/total) - count with vStepLog >= 50, count <= 2^17: every interval spans a whole step.",
    "rtb0_up": "proba = 0 needs count * T < total, but a symbol that reaches the rounding has count > lowThreshold = total >> tableLog, "
               "so count * T > total (step's truncation moves the product by less than 2^-44 of a unit).",
    "rtb0_down": "As rtb0_up: proba >= 1 wherever the restToBeat table is read.",
    "m2_total0_wrap": "total == 0 after the passes means every used symbol fits under lowOne, so there are at least T / 1.5 of them; "
                      "validity then forces total < T, lowThreshold = 0 and no -1 symbol: the T - used <= T / 3 increments end "
                      "before the first lap over at least 2 T / 3 positive symbols does.",
    "ncount_run_to_end": "The zero-run scan runs only while remaining > 1, i.e. a used symbol is still ahead: a valid norm's zero tail is "
                         "never scanned (the loop ends on remaining == 1, tag ncount_remaining1_early).",
}


# ---------------------------------------------------------------- FSE generators
def _fse_case(name, counts, maxsv, tablelog, low):
    """counts: maxsv + 1 values.  tablelog None: the one fse_optimal_table_log gives this shape."""
    cnt = np.zeros(64, np.uint32)
    cnt[:maxsv + 1] = np.asarray(counts, np.int64)[:maxsv + 1]
    total = int(cnt.sum())
    if tablelog is None:
        tablelog = optimal_table_log(FSE_MAXLOG.get(maxsv, 9), total, maxsv, 2)
    return FseCase(name, cnt, maxsv, total, tablelog, low)


def fse_valid(c):
    """The builders' domain: two used symbols at least, FSE_normalizeCount's argument check, a block's total."""
    return (c.total >= 2 and c.total <= LIT_MAX and int(c.count.max()) < c.total and 5 <= c.tablelog <= 9
            and c.tablelog >= min_table_log(c.total, c.maxsv))


def g_small(rng, n, T_):          # small uniform counts
    return rng.integers(0, int(rng.integers(2, 6)), n)


def g_dominant(rng, n, T_):       # one dominant symbol
    c = rng.integers(0, 3, n)
    c[int(rng.integers(0, n))] = int(rng.integers(50, 20000))
    return c


def g_equal(rng, n, T_):          # all equal, with holes now and then
    c = np.full(n, int(rng.integers(1, 40)))
    if rng.random() < 0.5:
        c[rng.random(n) < 0.2] = 0
    return c


def g_geometric(rng, n, T_):
    r = rng.uniform(1.1, 2.0)
    c = (r ** rng.permutation(np.minimum(np.arange(n), 28))).astype(np.int64)
    return np.maximum(c, rng.integers(0, 2, n))


def g_two_level(rng, n, T_):
    hi, lo = int(rng.integers(20, 3000)), int(rng.integers(1, 20))
    return np.where(rng.random(n) < rng.uniform(0.1, 0.9), hi, lo)


def g_round_up(rng, n, T_):
    """Most symbols at a probability just above k + rtb/2^20 (k small): each rounds up and the sum
    oversubscribes the table, the way into m2; holes and a few tiny counts mixed in."""
    k = int(rng.integers(1, 4))
    m = max(2, min(n, int(T_ / (k + rng.uniform(0.45, 0.6)))))
    base = int(rng.integers(1, 60))
    c = np.zeros(n, np.int64)
    idx = rng.permutation(n)[:m]
    c[idx] = base
    rest = [i for i in range(n) if c[i] == 0]
    for i in rest:
        u = rng.random()
        c[i] = 0 if u < 0.5 else int(rng.integers(1, max(2, base // 8 + 2))) if u < 0.8 else base * int(rng.integers(1, 4))
    return c


def g_low_heavy(rng, n, T_):
    """One or two large symbols over many symbols at or next to the low threshold total >> tableLog."""
    c = np.zeros(n, np.int64)
    big = int(rng.integers(200, 60000))
    c[int(rng.integers(0, n))] = big
    thr = max(1, big // T_)
    for i in range(n):
        if c[i] == 0 and rng.random() < 0.8:
            c[i] = max(0, thr + int(rng.integers(-1, 3)))
    return c


def g_runs(rng, n, T_):
    """Used symbols separated by zero runs of the lengths the NCount writer codes differently."""
    c = np.zeros(n, np.int64)
    i = 0
    while i < n:
        c[i] = int(rng.integers(1, 300))
        if rng.random() < 0.5 and i + 1 < n:
            c[i + 1] = int(rng.integers(1, 300))
            i += 1
        i += 1 + int(rng.choice(ZRUNS + (4, 7, 26, 28, 49, 52)))
    if rng.random() < 0.6:
        c[n - 1] = int(rng.integers(1, 300))
    return c


def g_sparse_ones(rng, n, T_):
    """Fewer sequences than table cells (total < T, so lowThreshold is 0): counts of 1 with a few
    2s and 3s and, half the time, holes.  Near total = T / 1.48 every 1 rounds up to 2 and m2
    hands out the whole table (its "all distributed" and total == 0 exits)."""
    c = np.ones(n, np.int64)
    for i in rng.permutation(n)[:int(rng.integers(0, 4))]:
        c[i] = int(rng.integers(2, 4))
    if rng.random() < 0.5:
        c[rng.permutation(n)[:int(rng.integers(1, max(2, n // 4)))]] = 0
    return c


def g_second_pass(rng, n, T_):
    """Many tiny symbols (each still costs a cell), one or two giants, and a few mediums between
    1.5 total / T and 1.5 total / (T - tiny): m2's second lowOne pass gives those 1."""
    c = np.zeros(n, np.int64)
    order = rng.permutation(n)
    ntiny = int(n * rng.uniform(0.4, 0.95))
    big = int(rng.integers(2000, 40000))
    c[order[:ntiny]] = rng.integers(1, max(2, big // (T_ * 8) + 2), ntiny)
    rest = order[ntiny:]
    if len(rest):
        c[rest[0]] = big
    for i in rest[1:]:
        c[i] = int(big * rng.uniform(1.0, 4.0) / T_) + 1 if rng.random() < 0.8 else int(big * rng.uniform(0.2, 1.0))
    return c


FSE_GENS = {"sparse_ones": g_sparse_ones, "second_pass": g_second_pass, "small": g_small, "dominant": g_dominant, "equal": g_equal, "geometric": g_geometric, "two_level": g_two_level,
            "round_up": g_round_up, "low_heavy": g_low_heavy, "runs": g_runs}


def fse_gen_case(gen, maxsv, tablelog, low, seed):
    """The case (generator, shape, seed) names; tablelog 0 = the optimal one.  None if the draw is outside the domain."""
    rng = np.random.default_rng([0x7AB1E, seed, maxsv, tablelog, low])
    c = FSE_GENS[gen](rng, maxsv + 1, 1 << (tablelog or FSE_MAXLOG.get(maxsv, 9)))
    c = np.minimum(np.asarray(c, np.int64), 60000)
    if c.sum() > LIT_MAX:
        c = c * LIT_MAX // (int(c.sum()) + 1)
    case = _fse_case(f"{gen}-sv{maxsv}-tl{tablelog}-low{low}-{seed}", c, maxsv, tablelog or None, low)
    return case if fse_valid(case) else None


def fse_hand_cases():
    """Constructions by hand (each comment: what it is for)."""
    out = []
    for low in (0, 1):
        # zero runs of every length the NCount writer treats differently, between two used symbols
        # (and one longer each: the writer counts the zeros after the first)
        for run in sorted(set(ZRUNS) | {n + 1 for n in ZRUNS}):
            maxsv = next(m for m in (35, 52, 63) if run + 2 < m + 1)
            c = np.zeros(maxsv + 1, np.int64)
            c[0], c[1 + run], c[maxsv] = 700, 300, 5
            out.append(_fse_case(f"hand-run{run}-sv{maxsv}-low{low}", c, maxsv, None, low))
            if low:  # ... and with a zero tail after it
                c[maxsv] = 0
                out.append(_fse_case(f"hand-run{run}-tail-sv{maxsv}-low{low}", c, maxsv, None, low))
        # every symbol but one below the low threshold; one low symbol; none
        for maxsv in (2, 12, 35, 63):
            c = np.ones(maxsv + 1, np.int64)
            c[maxsv // 2] = 4000
            out.append(_fse_case(f"hand-allbutone-sv{maxsv}-low{low}", c, maxsv, None, low))
            c = np.full(maxsv + 1, 300, np.int64)
            c[0] = 1
            out.append(_fse_case(f"hand-onelow-sv{maxsv}-low{low}", c, maxsv, None, low))
        # two symbols, the smallest alphabet; equal halves (tie for the largest) and a 1 : many split
        out.append(_fse_case(f"hand-halves-low{low}", [500, 500], 1, None, low))
        out.append(_fse_case(f"hand-1-to-many-low{low}", [1, 4000], 1, None, low))
        out.append(_fse_case(f"hand-many-to-1-low{low}", [4000, 1], 1, None, low))
        for tl in (5, 6, 7, 8, 9):
            out.append(_fse_case(f"hand-halves-tl{tl}-low{low}", [9, 9], 1, tl, low))
            out.append(_fse_case(f"hand-thirds-tl{tl}-low{low}", [7, 7, 7], 2, tl, low))
    return [c for c in out if fse_valid(c)]


# (generator, maxSV, tableLog or 0, useLowProbCount, seed): the first draws, in the grid's order
# over seeds 0-29, that meet each tag at up to three different shapes (the census in
# tests/test_table_cases.py re-proves what they reach)
FSE_FOUND = [
    ('sparse_ones', 1, 5, 1, 0), ('sparse_ones', 1, 9, 1, 0), ('sparse_ones', 2, 0, 0, 0), ('sparse_ones', 2, 0, 1, 0),
    ('sparse_ones', 2, 5, 0, 0), ('sparse_ones', 2, 6, 0, 0), ('sparse_ones', 2, 6, 1, 0), ('sparse_ones', 12, 0, 0, 0),
    ('sparse_ones', 12, 0, 1, 0), ('sparse_ones', 12, 5, 0, 0), ('sparse_ones', 12, 5, 1, 0), ('sparse_ones', 12, 6, 0, 0),
    ('sparse_ones', 12, 6, 1, 0), ('sparse_ones', 28, 0, 0, 0), ('sparse_ones', 28, 0, 1, 0), ('sparse_ones', 28, 5, 0, 0),
    ('sparse_ones', 28, 5, 1, 0), ('sparse_ones', 28, 6, 0, 0), ('sparse_ones', 28, 6, 1, 0), ('sparse_ones', 28, 7, 0, 0),
    ('sparse_ones', 28, 8, 1, 0), ('sparse_ones', 31, 0, 0, 0), ('sparse_ones', 31, 6, 1, 0), ('sparse_ones', 31, 7, 1, 0),
    ('sparse_ones', 35, 0, 1, 0), ('sparse_ones', 35, 6, 0, 0), ('sparse_ones', 35, 8, 0, 0), ('sparse_ones', 52, 7, 0, 0),
    ('sparse_ones', 63, 0, 0, 0), ('sparse_ones', 63, 0, 1, 0), ('sparse_ones', 42, 0, 1, 0), ('sparse_ones', 42, 7, 0, 0),
    ('sparse_ones', 42, 7, 1, 0), ('second_pass', 1, 0, 1, 0), ('second_pass', 1, 5, 1, 0), ('second_pass', 1, 6, 1, 0),
    ('second_pass', 2, 0, 1, 0), ('second_pass', 2, 5, 1, 0), ('second_pass', 2, 6, 1, 0), ('second_pass', 2, 7, 1, 0),
    ('second_pass', 28, 6, 1, 0), ('second_pass', 28, 7, 0, 0), ('second_pass', 63, 7, 0, 0), ('small', 12, 0, 1, 0), ('small', 28, 0, 1, 0),
    ('small', 28, 6, 1, 0), ('small', 28, 9, 1, 0), ('small', 35, 0, 1, 0), ('small', 52, 7, 1, 0), ('small', 63, 7, 0, 0),
    ('small', 42, 8, 0, 0), ('dominant', 28, 9, 1, 0), ('equal', 12, 6, 0, 0), ('equal', 12, 6, 1, 0), ('equal', 63, 9, 1, 0),
    ('geometric', 12, 9, 1, 0), ('runs', 28, 0, 1, 0), ('runs', 28, 7, 1, 0), ('runs', 31, 0, 1, 0), ('runs', 31, 9, 1, 0),
    ('runs', 63, 8, 0, 0), ('runs', 63, 8, 1, 0), ('second_pass', 31, 6, 1, 1), ('sparse_ones', 42, 0, 1, 2), ('round_up', 42, 0, 0, 2),
    ('sparse_ones', 42, 6, 1, 5), ('small', 52, 5, 1, 5), ('sparse_ones', 52, 6, 0, 8), ('small', 35, 0, 1, 8),
]


def fse_directed():
    out = fse_hand_cases()
    for g, sv, tl, low, seed in FSE_FOUND:
        c = fse_gen_case(g, sv, tl, low, seed)
        assert c is not None, (g, sv, tl, low, seed)
        out.append(c)
    return out


def fse_grid():
    out = []
    for gen in FSE_GENS:
        for maxsv in FSE_MAXSV + FSE_MAXSV_EXTRA:
            for tl in (0, 5, 6, 7, 8, 9):
                for low in (0, 1):
                    for seed in range(3):
                        c = fse_gen_case(gen, maxsv, tl, low, seed)
                        if c is not None:
                            out.append(c)
    return out


def fse_random(n=1000, seed=0x5EED7AB1):
    rng = np.random.default_rng(seed)
    out, gens = [], sorted(FSE_GENS)
    while len(out) < n:
        c = fse_gen_case(gens[int(rng.integers(len(gens)))], int(rng.choice(FSE_MAXSV + FSE_MAXSV_EXTRA)), int(rng.choice((0, 0, 5, 6, 7, 8, 9))),
                         int(rng.integers(2)), int(rng.integers(1000, 1 << 30)))
        if c is not None:
            out.append(c)
    return out


# ---------------------------------------------------------------- Huffman generators
def _huf_case(name, counts, maxbits, maxsv=None):
    cnt = np.zeros(256, np.uint32)
    counts = np.asarray(counts, np.int64)
    cnt[:len(counts)] = counts
    if maxsv is None:
        maxsv = int(np.nonzero(cnt)[0].max())
    if maxbits == "k2":
        maxbits = optimal_table_log(11, int(cnt.sum()), maxsv, 1)
    return HufCase(name, cnt, maxsv, maxbits)


def huf_valid(c):
    used = int((c.count != 0).sum())
    return used >= 2 and int(c.count.sum()) <= LIT_MAX and 1 <= c.maxbits <= 12 and used <= (1 << c.maxbits) and c.count[c.maxsv + 1:].sum() == 0


def _place(rng, vals, span):
    """vals at sorted random positions of [0, span), the last one at span - 1."""
    pos = np.sort(rng.permutation(span - 1)[:len(vals) - 1]).tolist() + [span - 1]
    c = np.zeros(span, np.int64)
    c[pos] = vals
    return c


def h_random(rng, used):
    return np.minimum(rng.zipf(rng.uniform(1.15, 2.5), used), 400).astype(np.int64) * int(rng.integers(1, 4))


def h_equal(rng, used):
    return np.full(used, int(rng.integers(1, 200)), np.int64)


def h_blocks(rng, used):        # blocks of equal counts: tie order decides the codes
    levels = rng.integers(1, 300, max(2, min(used // 4, int(rng.integers(2, 7)))))
    return rng.permutation(levels[np.arange(used) % len(levels)]).astype(np.int64)


def h_steep(rng, used):         # a steep head over a flat tail: the depth limit with many symbols to repay
    c = np.ones(used, np.int64)
    k = min(used, int(rng.integers(8, 20)))
    c[:k] = (rng.uniform(1.5, 2.2) ** np.arange(k)).astype(np.int64) + 1
    return rng.permutation(c)


def h_fibish(rng, used):        # Fibonacci-like growth with noise, capped to the block's literals
    c = [1, 1]
    while len(c) < used:
        c.append(min(c[-1] + c[-2] + int(rng.integers(-1, 2)), 3000 + int(rng.integers(0, 50))))
    return rng.permutation(np.maximum(np.array(c[:used], np.int64), 1))


HUF_GENS = {"random": h_random, "equal": h_equal, "blocks": h_blocks, "steep": h_steep, "fibish": h_fibish}


def huf_gen_case(gen, used, span, maxbits, seed):
    """used symbols spread over [0, span) (span - 1 = maxSV), maxbits 11, "k2" or a forced value."""
    rng = np.random.default_rng([0x40F, seed, used, span, 0 if maxbits == "k2" else maxbits])
    v = HUF_GENS[gen](rng, used)
    if v.sum() > LIT_MAX:
        v = np.maximum(v * LIT_MAX // (int(v.sum()) + used + 1), 1)
    c = _huf_case(f"{gen}-u{used}-s{span}-b{maxbits}-{seed}", _place(rng, v, span), maxbits)
    return c if huf_valid(c) else None


def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def gen_deepest():
    """The deepest tree a block's literals allow.  A leaf joins the chain (the one internal node)
    when it or its successor is no smaller than the node (HUF_buildCTable takes the internal node on
    a tie), so the slowest growth is c[k+1] = max(c[k], c[0] + ... + c[k-1]): 1, 1, 1, 2, 3, 5, ...
    with sums 1, 2, 3, 5, 8, ... (Fibonacci).  25 symbols total 121,393 <= 131,072 and give code
    length 24; a 26th symbol needs 75,025 more."""
    c = [1, 1]
    while sum(c) + max(c[-1], sum(c[:-1])) <= LIT_MAX:
        c.append(max(c[-1], sum(c[:-1])))
    return c


def huf_hand_cases():
    out = []
    for mb in (11, "k2", 8, 5):
        out.append(_huf_case(f"fib12-b{mb}", fib(12), mb))                 # depth exactly 11
        out.append(_huf_case(f"fib13-b{mb}", fib(13), mb))                 # depth 12: one level over
        out.append(_huf_case(f"fib13-rev-b{mb}", fib(13)[::-1], mb))
        out.append(_huf_case(f"fib20-b{mb}", fib(20), mb))
        out.append(_huf_case(f"deepest-b{mb}", gen_deepest(), mb))
        out.append(_huf_case(f"deepest-rev-holes-b{mb}", np.array([[v, 0, 0] for v in gen_deepest()[::-1]]).ravel()[:-2], mb))
        out.append(_huf_case(f"pow2-16-b{mb}", [1 << k for k in range(16)], mb))        # every node one short of the next leaf
        out.append(_huf_case(f"pow2-tie-16-b{mb}", [1] + [1 << k for k in range(15)], mb))  # every node ties the next leaf
        out.append(_huf_case(f"pow2-rev-14-b{mb}", [1 << k for k in range(13, -1, -1)], mb))
    for mb in (11, "k2", 2, 3):
        out.append(_huf_case(f"two-b{mb}", [5, 9], mb))
        out.append(_huf_case(f"two-far-b{mb}", [9] + [0] * 254 + [5], mb))
        out.append(_huf_case(f"three-b{mb}", [5, 9, 9], mb))
        out.append(_huf_case(f"three-eq-b{mb}", [7, 0, 7, 0, 0, 7], mb))
    for used in (4, 32, 33, 64, 65, 128, 129, 255, 256):
        need = highbit(used - 1) + 1
        for mb in (11, need):
            out.append(_huf_case(f"alleq-u{used}-b{mb}", np.full(used, 3), mb))
            out.append(_huf_case(f"iota-u{used}-b{mb}", np.arange(1, used + 1), mb))
    return [c for c in out if huf_valid(c)]


# (generator, used symbols, span, maxNbBits, seed): found by search, as FSE_FOUND
HUF_FOUND = [
    ('random', 2, 2, 11, 0), ('random', 2, 2, 'k2', 0), ('random', 2, 2, 1, 0), ('random', 2, 3, 11, 0), ('random', 2, 42, 11, 0),
    ('random', 3, 3, 11, 0), ('random', 3, 3, 'k2', 0), ('random', 3, 3, 2, 0), ('random', 32, 32, 11, 0), ('random', 32, 32, 'k2', 0),
    ('random', 32, 32, 5, 0), ('random', 32, 33, 6, 0), ('random', 32, 33, 8, 0), ('random', 32, 72, 6, 0), ('random', 33, 33, 11, 0),
    ('random', 33, 33, 'k2', 0), ('random', 33, 33, 6, 0), ('random', 64, 64, 11, 0), ('random', 64, 64, 'k2', 0), ('random', 64, 64, 6, 0),
    ('random', 65, 65, 11, 0), ('random', 65, 65, 'k2', 0), ('random', 65, 65, 7, 0), ('random', 128, 128, 11, 0),
    ('random', 128, 128, 'k2', 0), ('random', 128, 128, 7, 0), ('random', 129, 129, 11, 0), ('random', 129, 129, 'k2', 0),
    ('random', 129, 129, 8, 0), ('random', 255, 255, 11, 0), ('random', 255, 255, 'k2', 0), ('random', 255, 255, 8, 0),
    ('random', 256, 256, 11, 0), ('random', 256, 256, 'k2', 0), ('random', 256, 256, 8, 0), ('random', 5, 5, 4, 0), ('random', 12, 52, 5, 0),
    ('random', 20, 60, 6, 0), ('random', 100, 100, 7, 0), ('fibish', 12, 13, 11, 1),
]


def huf_directed():
    out = huf_hand_cases()
    for g, used, span, mb, seed in HUF_FOUND:
        c = huf_gen_case(g, used, span, mb, seed)
        assert c is not None, (g, used, span, mb, seed)
        out.append(c)
    return out


def huf_grid():
    out = []
    for gen in HUF_GENS:
        for used in HUF_USED + (5, 12, 20, 100, 200):
            for span in sorted({used, min(256, used + 1), min(256, used + 40), 256}):
                need = max(1, highbit(used - 1) + 1)
                for mb in [11, "k2"] + sorted({need, min(11, need + 1), 8} - {11}):
                    for seed in range(2):
                        c = huf_gen_case(gen, used, span, mb, seed)
                        if c is not None:
                            out.append(c)
    return out


def huf_random(n=1000, seed=0x5EED40F):
    rng = np.random.default_rng(seed)
    out, gens = [], sorted(HUF_GENS)
    while len(out) < n:
        used = int(rng.choice(HUF_USED)) if rng.random() < 0.4 else int(rng.integers(2, 257))
        span = int(rng.integers(used, 257))
        need = max(1, highbit(used - 1) + 1)
        mb = [11, "k2", int(rng.integers(need, 12))][int(rng.integers(3))]
        c = huf_gen_case(gens[int(rng.integers(len(gens)))], used, span, mb, int(rng.integers(1000, 1 << 30)))
        if c is not None:
            out.append(c)
    return out


# ---------------------------------------------------------------- census
def census(cases, oracle, tagger):
    """{tag: [case names]} over the cases, and the per-case results."""
    hit, results = {}, []
    for c in cases:
        r = oracle(c)
        results.append(r)
        for t in tagger(c, r):
            hit.setdefault(t, []).append(c.name)
    return hit, results

"""numpy model of the adaptive level selector's statistics and level rule (test infrastructure).

Written from the definitions in DESIGN.md ("Adaptive level selection"), not from any kernel or
host source.  Integer statistics are exact; the derived values are fp64, and `margin_ok` tells
whether they keep the distance from every threshold of the rule that makes an fp32
implementation's level and flags comparable."""
import functools

import numpy as np

SPEED, BALANCED, RATIO = 0, 1, 2
# rows: is_random | repetitive | compressibility > 0.7 | > 0.4 | otherwise; columns: SPEED, BALANCED, RATIO
LEVELS = ((1, 3, 3), (6, 12, 19), (5, 9, 16), (3, 6, 12), (1, 3, 6))
STATS_DTYPE = np.dtype([("sample_size", "<u4"), ("repeated_pairs", "<u4"), ("max_run_length", "<u4"), ("pattern_score", "<u4"),
                        ("unique_bytes", "<u4"), ("flags", "<u4"), ("entropy", "<f4"), ("repetition_ratio", "<f4"),
                        ("compressibility", "<f4"), ("level", "<i4")])


def integer_stats(data, sample_bytes=65536):
    """hist[256], repeated_pairs, max_run_length, pattern_score, unique_bytes of the first
    min(len(data), sample_bytes) bytes."""
    a = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data).reshape(-1)
    a = a[: min(len(a), sample_bytes)]
    n = len(a)
    hist = np.bincount(a, minlength=256).astype(np.int64)
    eq = a[:-1] == a[1:] if n >= 2 else np.zeros(0, bool)
    pairs = int(eq.sum())
    run = 0
    if pairs:
        # longest streak of equal neighbours + 1 = longest run
        z = np.flatnonzero(~np.concatenate([[False], eq, [False]]))
        run = min(int(np.diff(z).max()), 256)
    score = 0
    if n >= 5:
        m = n - 4  # i in [0, n - 4)
        score += int(((a[:m] == a[2 : m + 2]) & (a[1 : m + 1] == a[3 : m + 3])).sum())
        k = n - 8  # i + 8 < n; the four bytes at i + 4 end at i + 7
        if k > 0:
            k = min(k, m)
            e4 = a[: n - 4] == a[4:]
            score += 2 * int((e4[:k] & e4[1 : k + 1] & e4[2 : k + 2] & e4[3 : k + 3]).sum())
    return {"n": n, "hist": hist, "repeated_pairs": pairs, "max_run_length": run, "pattern_score": score,
            "unique_bytes": int((hist != 0).sum())}


def derive(s, preference=BALANCED):
    """The derived values (fp64), the flags, the branch of the rule and the level."""
    n = s["n"]
    if n == 0:
        return {"entropy": 0.0, "repetition_ratio": 0.0, "compressibility": 0.0, "has_patterns": False, "is_random": False,
                "branch": None, "level": 3, "margin_ok": True}
    p = s["hist"][s["hist"] != 0] / n
    entropy = float(-(p * np.log2(p)).sum())
    rep = s["repeated_pairs"] / n
    comp = min(max(0.6 * (1.0 - entropy / 8.0) + 0.4 * rep, 0.0), 1.0)
    has_patterns = s["pattern_score"] > n // 100
    is_random = entropy > 7.5 and not has_patterns
    if is_random:
        branch = 0
    elif rep > 0.5 or s["max_run_length"] > 100:
        branch = 1
    elif comp > 0.7:
        branch = 2
    elif comp > 0.4:
        branch = 3
    else:
        branch = 4
    # a repetition ratio of exactly 1/2 is exact in fp32 and fp64 alike: the comparison cannot differ
    rep_ok = abs(rep - 0.5) >= 0.01 or 2 * s["repeated_pairs"] == n
    margin_ok = abs(entropy - 7.5) >= 0.05 and abs(comp - 0.7) >= 0.01 and abs(comp - 0.4) >= 0.01 and rep_ok
    return {"entropy": entropy, "repetition_ratio": rep, "compressibility": comp, "has_patterns": bool(has_patterns),
            "is_random": bool(is_random), "branch": branch, "level": LEVELS[branch][preference], "margin_ok": margin_ok}


def analyze(data, preference=BALANCED, sample_bytes=65536):
    s = integer_stats(data, sample_bytes)
    s.update(derive(s, preference))
    return s


# ---- the inputs the host and GPU tests share -------------------------------------------------
NAMES = ["MIX", "RANDOM", "SYM16", "TEXT", "JSON", "CSV", "SENSOR", "zeros", "01", "0123", "random_run300", "period50"]
# the branch each takes (rows of LEVELS): together all five
BRANCH = {"RANDOM": 0, "zeros": 1, "random_run300": 1, "period50": 2, "01": 3, "0123": 3}
SEED = 0x5EED0003


@functools.lru_cache(maxsize=None)
def named_inputs():
    """One 64 KiB chunk per name: the generator's kinds at SEED, and five synthetic ones."""
    import zh_testlib as T

    d = {k: T.gen(getattr(T, "DG_" + k), 1, SEED, 65536) for k in NAMES[:7]}
    d["zeros"] = np.zeros(65536, np.uint8)
    d["01"] = np.tile(np.array([0, 1], np.uint8), 32768)
    d["0123"] = np.tile(np.array([0, 1, 2, 3], np.uint8), 16384)
    d["random_run300"] = random_with_run(65536, 30000, 300)
    d["period50"] = period50_tile()
    return d


def period50_tile(n=65536):
    """Zeros with ones at 3, 7, ..., 47 and 49 of every 50 bytes: repetition 0.48, compressibility 0.73."""
    t = np.zeros(50, np.uint8)
    t[3:48:4] = 1
    t[49] = 1
    return np.tile(t, (n + 49) // 50)[:n].copy()


def random_with_run(n, start, length, seed=0x5EED0A01, value=0x55):
    """Random bytes with `length` equal bytes at `start`; the neighbours differ from `value`."""
    a = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    a[start : start + length] = value
    if start:
        a[start - 1] = value ^ 0xFF
    if start + length < n:
        a[start + length] = value ^ 0xFF
    return a

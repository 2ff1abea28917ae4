"""Directed encoder inputs (test infrastructure): small seeded inputs, each built to drive the
compressor into one named path of the entropy stage that the corpora never reach -- sequence
tables in RLE mode, RLE literals, raw literals with the 3-byte header, Huffman literals with
direct weights or a single stream, and the literal / sequence counts on either side of every
header-size boundary.  tests/test_encoder_paths.py proves on the CPU (oracle frames walked by
zh_frames) that the paths are reached; tests/test_gpu_encoder_paths.py runs the same inputs
through the GPU compressor.

Only numpy is used.  The seeds below were found by searching each builder's
seeds with the oracle; the inputs are the same at every level (a seed was kept when it reaches
its path at all of LEVELS), and tests/test_encoder_paths.py re-proves what they reach."""
import numpy as np


def _rng(seed):
    return np.random.default_rng(seed)


def copies(seed, alpha, base, reps, copy, fresh, equal=False, lo=0, band=None):
    """A base of `base` bytes over `alpha` symbols, then `reps` times [a copy of `copy` bytes
    from a random place of the base][`fresh` fresh bytes].  Ranges (lo, hi) are drawn per item
    with the seeded generator; equal=True draws the copy length once; band=(lo, hi) keeps every
    copy's distance inside it (one offset code)."""
    r = _rng(seed)
    pick = lambda x: int(r.integers(x[0], x[1] + 1)) if isinstance(x, tuple) else x  # noqa: E731
    b = r.integers(lo, lo + alpha, pick(base), dtype=np.uint8)
    parts, cl, pos = [b], pick(copy), len(b)
    for _ in range(pick(reps)):
        if not equal:
            cl = pick(copy)
        s0, s1 = (0, len(b) - cl) if band is None else (max(0, pos - band[1]), min(len(b) - cl, pos - band[0]))
        if s1 < s0:
            break
        s = int(r.integers(s0, s1 + 1))
        parts += [b[s:s + cl], r.integers(lo, lo + alpha, pick(fresh), dtype=np.uint8)]
        pos += len(parts[-1]) + cl
    return np.concatenate(parts)


def one_code(seed, alpha, reps, ll, copy, dist, equal=False):
    """`reps` times [`ll` fresh bytes over `alpha` symbols][a copy of `copy` bytes from `dist`
    bytes back], then `ll` fresh bytes.  With ll inside one literal-length code (128-255: code
    26), dist inside one offset code and, with equal=True, one copy length, every sequence has
    the same LL, OF and ML code."""
    r = _rng(seed)
    pick = lambda x: int(r.integers(x[0], x[1] + 1)) if isinstance(x, tuple) else x  # noqa: E731
    out = list(r.integers(0, alpha, pick(ll), dtype=np.uint8))
    cl = pick(copy)
    for _ in range(pick(reps)):
        if not equal:
            cl = pick(copy)
        d = min(max(pick(dist), cl), len(out))
        out += out[len(out) - d:len(out) - d + cl]
        out += list(r.integers(0, alpha, pick(ll), dtype=np.uint8))
    return np.array(out, np.uint8)


def spikes(seed, n, gap, fill=0, spike=0x78):
    """`fill` bytes with a single `spike` byte every gap[0]..gap[1] bytes: thousands of short
    matches that run across the spikes (a 2-byte sequence count) and only a handful of literals
    per block (raw with the 1-byte header, one Huffman stream, or RLE when all are spikes)."""
    r = _rng(seed)
    a = np.full(n, fill, np.uint8)
    p = int(r.integers(gap[0], gap[1] + 1))
    while p < n:
        a[p] = spike
        p += int(r.integers(gap[0], gap[1] + 1))
    return a


def symbols(seed, n, alpha, lo=65):
    return _rng(seed).integers(lo, lo + alpha, n, dtype=np.uint8)


def literals(seed, nlit, alpha, seg=1500, copy=40, back=700):
    """`nlit` fresh bytes over `alpha` symbols in runs of at most `seg`, each run but the last
    followed by a copy of `copy` bytes from min(`back`, all) bytes back (overlapping itself when
    copy > back); a single run is followed by its copy.  When the parse takes exactly the copies,
    the block has `nlit` literals."""
    r = _rng(seed)
    out, left = [], nlit
    while left:
        k = min(seg, left)
        out += list(r.integers(0, alpha, k, dtype=np.uint8))
        left -= k
        if left or nlit <= seg:
            b = min(back, len(out))
            for _ in range(copy):
                out.append(out[-b])
    return np.array(out, np.uint8)


def many_seqs(seed, nseq, copy=8, fresh=3):
    """A random base, then `nseq` times [`copy` bytes from a fresh place of the base][`fresh`
    random bytes]: about nseq sequences."""
    r = _rng(seed)
    b = r.integers(0, 256, nseq * copy + 64, dtype=np.uint8)
    parts = [b]
    for i in range(nseq):
        parts += [b[i * copy:(i + 1) * copy], r.integers(0, 256, fresh, dtype=np.uint8)]
    return np.concatenate(parts)


def rows(seed, n, width=64):
    """`width`-byte rows, each the previous one with one byte changed: every match has the same
    offset, so the blocks after the first begin with repeated offsets."""
    r = _rng(seed)
    row, out = r.integers(0, 256, width, dtype=np.uint8), []
    for _ in range(n // width):
        row = row.copy()
        row[int(r.integers(0, width))] = int(r.integers(0, 256))
        out.append(row)
    return np.concatenate(out)


def pieces(seed, piece, count=None, span=32768, spike=0x78):
    """32 KiB of random bytes (block 1 of a three-block frame), then a 32 KiB block 2 of `count`
    times [`piece` bytes from a place in the last `span` bytes of block 1 that is used once][one
    `spike` byte] and spikes to its end (every match comes from the history or from the run of
    spikes, every literal is a spike; the block's last bytes, which are never matched, too), then
    64 zeros (block 3).  count None: as many as fit before the last 16 bytes."""
    r = _rng(seed)
    b = r.integers(0, 256, 32768, dtype=np.uint8)
    b[b == spike] = spike + 1
    n = (32768 - 16) // (piece + 1) if count is None else count
    slots = 32768 - span + piece * r.permutation(span // piece)[:n]
    blk = np.full(32768, spike, np.uint8)
    for i, s in enumerate(slots):
        blk[i * (piece + 1):i * (piece + 1) + piece] = b[s:s + piece]
    return np.concatenate([b, blk, np.zeros(64, np.uint8)])


# builder name -> (function, fixed arguments); a case is (builder name, seed)
BUILDERS = {
    # literal lengths 70-120 share LL code 25 and copies of 12-14 bytes sit in ML codes 9-11:
    # some seeds give one LL code (ll_rle), some one ML code (ml_rle)
    "a24": (copies, dict(alpha=24, base=(120, 600), reps=(3, 11), copy=(12, 14), fresh=(70, 120))),
    # equal-length copies: one ML code (ml_rle); 600-900 random literals between them add up to
    # more than 4095 raw literals (lit_raw_h3)
    "eq256": (copies, dict(alpha=256, base=(1000, 2000), reps=(6, 9), copy=(200, 400), fresh=(600, 900), equal=True)),
    "eq8": (copies, dict(alpha=64, base=(3000, 4000), reps=(8, 30), copy=8, fresh=(40, 120), equal=True)),
    "eq12": (copies, dict(alpha=64, base=(3000, 4000), reps=(4, 12), copy=12, fresh=(70, 120), equal=True)),
    # two long copies inside random bytes
    "rand2": (copies, dict(alpha=256, base=(20000, 30000), reps=2, copy=(2000, 6000), fresh=(8000, 12000))),
    "spike_s": (spikes, dict(n=131072, gap=(40, 300))),
    "spike_l": (spikes, dict(n=131072, gap=(6, 8))),
    # every copy 1030-2040 bytes back: offset code 10 throughout (of_rle alone)
    "band24": (copies, dict(alpha=24, base=(1040, 1100), reps=(3, 7), copy=(12, 14), fresh=(70, 120), band=(1030, 2040))),
    "band64": (copies, dict(alpha=64, base=(1040, 1100), reps=(3, 7), copy=(12, 14), fresh=(70, 120), band=(1030, 2040))),
    # every literal run in LL code 26 and every distance in offset code 7 (ll_rle + of_rle); with
    # one copy length, ML too (all three tables in RLE mode)
    "code24": (one_code, dict(alpha=24, reps=(3, 9), ll=(130, 250), copy=(12, 14), dist=(128, 250))),
    "code64": (one_code, dict(alpha=64, reps=(3, 9), ll=(130, 250), copy=(12, 14), dist=(128, 250))),
    "code64eq": (one_code, dict(alpha=64, reps=(3, 9), ll=(130, 250), copy=(9, 16), dist=(128, 250), equal=True)),
    "pieces5": (pieces, dict(piece=5)),
    "pieces6": (pieces, dict(piece=6)),
    "pieces7": (pieces, dict(piece=7)),
    "pieces8_100": (pieces, dict(piece=8, count=100, span=1600)),
    "pieces12_300": (pieces, dict(piece=12, count=300, span=4800)),
    "sym5_700": (symbols, dict(n=700, alpha=5)),
    "sym2_200": (symbols, dict(n=200, alpha=2)),
    "sym24_282": (symbols, dict(n=282, alpha=24)),
    # symbol values from 0: a short weight list, written directly
    "lo5_700": (symbols, dict(n=700, alpha=5, lo=0)),
    "lo16_200": (symbols, dict(n=200, alpha=16, lo=0)),
    "lo12_150": (symbols, dict(n=150, alpha=12, lo=0)),
    "rows": (rows, dict(n=114688)),
}


def build(name, seed, **kw):
    fn, fixed = BUILDERS[name]
    return fn(seed, **{**fixed, **kw})


def _lit(n, alpha, **kw):
    return ("lits_%d_a%d" % (n, alpha), literals, 1, dict(nlit=n, alpha=alpha, **kw))


# (name, builder, seed, arguments); the seeds are the first ones the oracle confirms at every
# level of LEVELS for the path named (tests/test_encoder_paths.py re-checks them)
LEVELS = (1, 2, 3, 5, 9)
CASES = [(n, BUILDERS[b][0], s, BUILDERS[b][1]) for n, b, s in (
    ("ll_of_rle", "code64", 2), ("ll_of_rle_a24", "code24", 2), ("all_rle", "code64eq", 2), ("all_rle_b", "code64eq", 4),
    ("ml_rle_a24", "a24", 21), ("ml_rle_eq12", "eq12", 7), ("ml_rle_eq8", "eq8", 1), ("ll_rle_a24", "a24", 27),
    ("of_rle_band", "band64", 2), ("of_rle_band_a24", "band24", 5),
    ("raw_h3_eq256", "eq256", 1), ("raw_h3_rand2", "rand2", 5),
    ("rle_lits_100", "pieces8_100", 4), ("rle_lits_300", "pieces12_300", 3), ("rle_lits_4679", "pieces6", 1), ("rle_lits_5458", "pieces5", 1),
    ("spikes_sparse", "spike_s", 1), ("spikes_dense", "spike_l", 1),
    ("direct_4stream", "lo5_700", 1), ("direct_1stream", "lo12_150", 1), ("direct_1stream_b", "lo16_200", 2), ("fse_1stream", "lo16_200", 1),
    ("sym5_700", "sym5_700", 1), ("sym2_200", "sym2_200", 1), ("sym24_282", "sym24_282", 1),
    ("rows_4_blocks", "rows", 1),
)]
# the literal count on either side of every size boundary of the literals header: raw 1 / 2 / 3
# bytes at 31|32 and 4095|4096, never compressed up to 63, one Huffman stream up to 255, Huffman
# headers of 3 / 4 / 5 bytes at 1023|1024 and 16383|16384
CASES += [_lit(31, 256, copy=300, back=31), _lit(32, 256, copy=300, back=32), _lit(63, 8, copy=300, back=63), _lit(64, 8, copy=300, back=64),
          _lit(255, 16), _lit(256, 16), _lit(1023, 32), _lit(1024, 32), _lit(4095, 256, copy=100), _lit(4096, 256, copy=100),
          _lit(4095, 64), _lit(4096, 64), _lit(16383, 64), _lit(16384, 64), _lit(16383, 256), _lit(16384, 256)]
LITERAL_BOUNDARIES = (31, 32, 63, 64, 255, 256, 1023, 1024, 4095, 4096, 16383, 16384)
# the sequence count on either side of its 1 / 2 byte boundary, and two sequences with the same
# three codes (select_encoding_type takes the predefined tables, not RLE, up to two sequences)
CASES += [("nseq_127", many_seqs, 1, dict(nseq=127)), ("nseq_128", many_seqs, 3, dict(nseq=128)),
          ("two_same_codes", one_code, 1, dict(alpha=64, reps=2, ll=(130, 250), copy=12, dist=(128, 250), equal=True)),
          ("random_1000", symbols, 1, dict(n=1000, alpha=256, lo=0))]


def cases(level=3):
    """[(name, uint8 array)]: the same inputs at every level (each at most 128 KiB)."""
    assert level in LEVELS
    return [(n, np.ascontiguousarray(fn(seed, **kw))) for n, fn, seed, kw in CASES]

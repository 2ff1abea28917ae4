"""End-to-end inputs (at most 64 KiB, one block) whose oracle frames take FSE_normalizeM2 in a
sequence table through the real K2 path: the block's own LL, OF or ML histogram sends
fse_normalize_wave to its serial fall-back (test infrastructure).  Found with the oracle's branch
trace (SEQ_M2_LL / SEQ_M2_OF / SEQ_M2_ML, oracle/zstd_oracle.c); tests/test_table_cases.py asserts
on the CPU which input reaches m2 in which table at which level, tests/test_gpu_tables.py compresses
them on the GPU.  Only numpy is used."""
import numpy as np

LEVELS = (1, 2, 3, 5, 9)


def pieces(seed, nbase, npieces, ml_lo, ml_span, lit_lo, lit_mul, lit_span, gap=3):
    """`nbase` random bytes, then `npieces` pieces: piece i copies ml = ml_lo + i mod ml_span bytes
    of the base from position pos, after which pos advances by ml + gap (wrapping), and is
    followed by lit_lo + (lit_mul i) mod lit_span fresh random bytes.  The match lengths, literal
    lengths and distances spread over many codes with small, nearly equal counts: probabilities
    of 1.5 to 3.5 cells that all round up and oversubscribe the table."""
    r = np.random.default_rng(seed)
    base = r.integers(0, 256, nbase, dtype=np.uint8)
    parts, pos = [base], 0
    for i in range(npieces):
        ml = ml_lo + i % ml_span
        if pos + ml > nbase:
            pos = 0
        parts.append(base[pos:pos + ml])
        pos += ml + gap
        parts.append(r.integers(0, 256, lit_lo + (lit_mul * i) % lit_span, dtype=np.uint8))
    return np.concatenate(parts)[:65536]


def far(seed, nseq, codes, ml=6, lit=2):
    """Random bytes, then `nseq` copies of `ml` bytes from a distance inside offset code
    codes[i mod len(codes)] (code k: distances [2^k, 2^(k+1)) less the 3 of Offset_Value), each
    followed by `lit` fresh bytes: an offset histogram that is flat over the codes.  Twelve codes
    four times each under a 32-cell table are 2.7 cells each, which all round up to 3."""
    r = np.random.default_rng(seed)
    out = r.integers(0, 256, 65536, dtype=np.uint8)
    n = (1 << (max(codes) + 1)) + 16
    for i in range(nseq):
        if n + ml + lit > 65536:
            break
        k = codes[i % len(codes)]
        d = int(r.integers(1 << k, 1 << (k + 1))) - 3
        d = min(max(d, ml + 1), n)
        out[n:n + ml] = out[n - d:n - d + ml]
        n += ml + lit
    return out[:n].copy()


def cases():
    """[(name, bytes)]; the parameters are the first the search confirmed per table."""
    return [
        ("ml_pieces_68", pieces(76, 8192, 68, 7, 30, 2, 1, 17)),
        ("ml_pieces_143", pieces(56, 4096, 143, 6, 34, 0, 3, 6)),
        ("ll_ml_pieces_88", pieces(89, 4096, 88, 6, 21, 3, 7, 17)),
        ("ll_pieces_578", pieces(8, 4096, 578, 4, 10, 3, 11, 24)),
        ("ll_pieces_424", pieces(20, 4096, 424, 5, 21, 0, 5, 19)),
        ("of_far_36", far(1, 36, tuple(range(2, 14)), 6, 2)),
        # the control: many codes, no table oversubscribed at any level
        ("none_pieces_1000", pieces(7, 16384, 1000, 5, 45, 1, 7, 33)),
    ]


# {name: {level: tables whose normalisation takes m2}}, as the oracle's trace shows it
# (tests/test_table_cases.py::test_inputs_reach_m2 re-proves every entry, absent ones included)
REACH = {
    "ml_pieces_68": {1: "ML", 2: "ML", 3: "ML", 5: "ML", 9: "ML"},
    "ml_pieces_143": {1: "ML", 2: "ML", 3: "ML", 5: "ML", 9: "ML"},
    "ll_ml_pieces_88": {1: "LL", 5: "LL ML", 9: "LL ML"},
    "ll_pieces_578": {2: "LL", 3: "LL"},
    "ll_pieces_424": {1: "LL", 2: "ML", 3: "LL"},
    "of_far_36": {5: "OF", 9: "OF"},
    "none_pieces_1000": {},
}
# Tables no searched input sends to m2 at a level, with the bounds of the search.
UNREACHED = {
    "OF at levels 1-3": "2,000 far() inputs (seeds 1-29, 36-60 sequences over twelve codes from 3 or 4, match length 8-16) and 4,000 "
                        "random-code ones: the fast matcher drops a few of the short far matches and the histogram is no longer flat. "
                        "Levels 5 and 9 (the deep matcher) take every one: of_far_36.",
}

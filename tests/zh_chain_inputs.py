"""Directed inputs for the encoder's FSE chain and packing kernels (test infrastructure): small
seeded one-block inputs (at most 64 KiB), each kept because the model of the chain kernel
(tests/zh_chain_model.py) run over the oracle's level-3 parse shows that it drives the kernel
into a named state -- a chain that needs no repair, one that needs all 20 rounds, re-runs that
merge in the middle of a segment, at its last batch or not at all, dead tails, short and full
warm-ups -- or because its sequence count sits on one side of a geometry edge of the two
kernels.  tests/test_chain_model.py re-proves on the CPU what every case reaches;
tests/test_gpu_chain.py compresses the same inputs on the GPU.

Only numpy is used.  The builders of zh_edge_inputs are reused; the seeds and counts below are
the first ones per builder that the tracer confirmed."""
import numpy as np

from zh_edge_inputs import LEVELS, many_seqs, one_code, rows, spikes  # noqa: F401 (LEVELS: the levels the GPU test runs)


def cycle(seed, nseq, places, copy=8, fresh=3, head=0, last=False, ramp=False, echo=False):
    """`places` slots of random bytes below 128, then `nseq` times [the first bytes of slot k mod
    places][literals of 128 and above whose first and last byte differ between two uses of a
    slot]: no match runs on into the literals or back over them, so the parse takes these
    sequences and no others (but for a match the hash tables lose).
      copy   the match length: one number, (lo, hi) for lo + slot mod (hi - lo + 1), or a list
             with a length per slot
      fresh  the literal count: one number, or (lo, hi) drawn per sequence
      ramp   adds the round (k / places) to the literal count: every distance is one more than
             the one before, so no offset repeats and all share one offset code
      echo   the slots are written twice: the parse starts with one long match at distance =
             literal length = places * slot size (the first tile of 256 positions sees no match)
    With one match length, one literal count or one offset code, that table's chain has one
    dominant code, its step map is close to a permutation and trajectories never merge.  The
    first `head` sequences are odd (1-3 bytes shorter, 1-2 literals fewer, the slot half a round
    away) and with last=True the last one is (1 byte, 1 literal): the table is not RLE; its
    dominant code is not its lowest, whose first state is stT[0], the warm-up's start; step 0's
    code differs from both; and every other odd code is in the chain's last segment."""
    r = np.random.default_rng(seed)
    lens = [copy] * places if isinstance(copy, int) else [copy[0] + j % (copy[1] - copy[0] + 1) for j in range(places)] if isinstance(copy, tuple) \
        else [copy[j % len(copy)] for j in range(places)]
    slot = max(lens) + 4
    base = r.integers(0, 128, places * slot, dtype=np.uint8)
    parts = [base, base] if echo else [base]
    for k in range(nseq):
        cut = (1 + k % 3, 1 + k % 2) if k < head else (1, 1) if last and k == nseq - 1 else (0, 0)
        j = (k + (places // 2 if k < head else 0)) % places
        parts.append(base[j * slot:j * slot + lens[j] - cut[0]])
        nf = (fresh if isinstance(fresh, int) else int(r.integers(fresh[0], fresh[1] + 1))) + (k // places if ramp else 0) - cut[1]
        lit = r.integers(192, 256, max(nf, 1), dtype=np.uint8)
        lit[0] = 128 + k % 64
        lit[-1] = 128 + (k + (len(lit) > 1)) % 64
        parts.append(lit)
    return np.concatenate(parts)


# the first match length of ML codes 2 .. 39, one per slot: every code nbSeq / 38 times, none as
# often as nbSeq / 32, so select_encoding_type takes the predefined table
ML_LENGTHS = [c + 3 for c in range(2, 32)] + [35, 37, 39, 41, 43, 47, 51, 59]


def dense(seed, n, places, copy=5):
    """`places` random pieces of `copy` bytes, then pieces again with no literal between them, in
    an order in which no pair of neighbours comes twice (piece k (1 + k / places) mod places):
    every piece is a match of the minimum length with an offset of its own, the most sequences
    the parse can be driven to."""
    r = np.random.default_rng(seed)
    base = r.integers(0, 256, (places, copy), dtype=np.uint8)
    k = np.arange((n - places * copy) // copy)
    return np.concatenate([base.reshape(-1), base[(k * (1 + k // places)) % places].reshape(-1)])[:n]


def wide(seed, nseq, base=4096, gap=20000, copy=60, fresh=(260, 400)):
    """`base` random bytes, `gap` zeros (their positions share one hash key, so the base stays in
    the tables), then `nseq` times [`copy` bytes from a random place of the base][a long run of
    fresh bytes]: literal lengths of 8-9 extra bits and offsets of 14-15, the widest 64-step
    appends of the packing kernel in this set."""
    r = np.random.default_rng(seed)
    b = r.integers(0, 128, base, dtype=np.uint8)
    parts = [b, np.zeros(gap, np.uint8)]
    for _ in range(nseq):
        p = int(r.integers(0, base - copy))
        parts += [b[p:p + copy], r.integers(128, 256, int(r.integers(fresh[0], fresh[1] + 1)), dtype=np.uint8)]
    return np.concatenate(parts)


def _count(n, nseq=None, seed=1, places=31):
    # (long copies where there are few: the block must still compress)
    return ("nseq_%d" % n, cycle, seed, dict(nseq=nseq or n, places=places, copy=40 if n < 63 else 8, head=min(n // 4, 5), last=n > 8))


# the sequence count on both sides of every geometry edge: 21 segments (20 | 21 | 22), one 16-step
# batch per segment (16 | 17), K4's 64-step chunks (63 | 64 | 65, 128 | 129), ZH_K3_SEGLEN 16 | 32 |
# 48 (336 | 337, 672 | 673) and the full warm-up of 128 steps (2,687 | 2,688 | 2,689)
EXACT = (1, 2, 16, 17, 20, 21, 22, 63, 64, 65, 128, 129, 335, 336, 337, 672, 673, 2687, 2688, 2689)
# (name, builder, seed, arguments); "nseq_N" has exactly N sequences
CASES = [_count(n) for n in EXACT if n < 2687] + [
    # one literal length and one match length throughout, odd ones in the last segment and at step 0:
    # the LL and ML chains take all 20 rounds at L = 128 (exactly 21 full segments)
    ("nseq_2688", cycle, 3, dict(nseq=2688, places=125, head=5, last=True)),
    ("nseq_2687", cycle, 2, dict(nseq=2688, places=125, head=5, last=True)),
    ("nseq_2689", cycle, 1, dict(nseq=2689, places=125, head=5, last=True)),
    # every distance one more than the one before, all of offset code 11: OF and ML, 20 rounds at L = 128
    ("ramp_2688", cycle, 1, dict(nseq=2688, places=250, fresh=1, head=3, last=True, ramp=True)),
    ("cycle_1344", cycle, 3, dict(nseq=1344, places=61, head=5, last=True)),
    ("ramp_1344", cycle, 1, dict(nseq=1344, places=234, fresh=1, head=3, last=True, ramp=True)),
    ("cycle_4200", cycle, 1, dict(nseq=4200, places=199, head=5, last=True)),
    # the inputs that showed the gap: chains that never merge in ordinary data
    ("many_2000", many_seqs, 5, dict(nseq=2000)), ("many_1000_a", many_seqs, 1, dict(nseq=1000, copy=12, fresh=5)),
    ("many_1000_b", many_seqs, 8, dict(nseq=1000, copy=12, fresh=5)), ("spikes_6_8", spikes, 18, dict(n=65536, gap=(6, 8))),
    # chains whose guesses are all right
    ("rows_16", rows, 3, dict(n=65536, width=16)), ("spikes_sparse", spikes, 8, dict(n=16384, gap=(40, 300))),
    ("copies_12", one_code, 3, dict(alpha=256, reps=400, ll=(3, 40), copy=12, dist=(12, 6000), equal=True)),
    # every ML code from 2 to 39 equally often: the predefined ML table on a long chain
    ("ml_predefined_672", cycle, 3, dict(nseq=672, places=76, copy=ML_LENGTHS, fresh=2)),
    # one table in RLE mode beside two FSE tables, nbSeq > 336
    ("ll_rle_340", cycle, 1, dict(nseq=340, places=3, copy=(40, 42), fresh=(132, 150), echo=True)),
    ("ml_rle_400", cycle, 1, dict(nseq=400, places=37, copy=8, fresh=(1, 4))),
    ("of_rle_400", many_seqs, 1, dict(nseq=400, copy=12, fresh=5)),
    # the most sequences, and the widest appends
    ("dense_127", dense, 1, dict(n=65536, places=127)), ("wide_70", wide, 1, dict(nseq=70)),
]


def cases():
    """[(name, uint8 array)], each at most 64 KiB"""
    return [(n, np.ascontiguousarray(fn(seed, **kw))) for n, fn, seed, kw in CASES]

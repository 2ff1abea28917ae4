"""Inputs of the deep matcher's raw-output tests (tests/test_gpu_deep.py, the forced fix-up worker
and the CPU-side tests/test_deep_inputs.py): the oracle's deep parse and per-position matches
through ctypes, the path function of the library, the LAZY2 census, and the case builders.  A case
is (name, prefix bytes, block bytes, device byte offset); the staged buffer is prefix + block."""
import ctypes

import numpy as np

import zh_testlib as T

BLOCK = 65536
DEEP_PRE, MAXOFF, HASH_READ, MAX_MATCH = 65536, 65535, 8, 64  # ZH_DEEP_PRE, ZH_DEEP_MAXOFF, ZH_HASH_READ, ZH_MAX_MATCH
HB = 8192  # positions per chain-building round (zh_lz_deep.hip)
DEMAND, LDS_BYTES, LDS_LINKS, SLOT = range(4)  # DEEP_PATH_* (zh_lz_deep.hip)
EMPTY = np.zeros(0, np.uint8)


def u8(x):
    return np.ascontiguousarray(np.frombuffer(bytes(x), np.uint8) if not isinstance(x, np.ndarray) else x, dtype=np.uint8)


# ---- the oracle ---------------------------------------------------------------------------------
def oracle_parse(pre, blk, depth):
    """orc_lz_parse_deep over prefix + block: [(ll, ml, off)], trailing literals."""
    O = T.oracle()
    buf = np.concatenate([u8(pre), u8(blk)])
    seq = (ctypes.c_uint32 * (3 * (len(blk) // 5 + 2)))()
    last = ctypes.c_uint32(0)
    O.orc_lz_parse_deep.restype = ctypes.c_size_t
    ns = O.orc_lz_parse_deep(buf.ctypes.data_as(T.vp), ctypes.c_uint32(len(pre)), ctypes.c_uint32(len(buf)), ctypes.c_uint32(depth), seq,
                             ctypes.byref(last))
    return [(seq[3 * i], seq[3 * i + 1], seq[3 * i + 2]) for i in range(ns)], last.value


def oracle_matches(pre, blk, depth):
    """orc_deep_matches over prefix + block: (len, off) per block position."""
    O = T.oracle()
    buf = np.concatenate([u8(pre), u8(blk)])
    n = len(buf)
    ln = np.zeros(n + 3, np.uint8)
    off = np.zeros(n + 3, np.uint32)
    O.orc_deep_matches.restype = None
    O.orc_deep_matches(buf.ctypes.data_as(T.vp), ctypes.c_uint32(len(pre)), ctypes.c_uint32(n), ctypes.c_uint32(depth), ln.ctypes.data_as(T.vp),
                       off.ctypes.data_as(T.vp))
    return ln[len(pre):n].astype(np.int64), off[len(pre):n].astype(np.int64)


def is_rle(blk):
    return len(blk) >= 2 and bool((blk == blk[0]).all())


def gain(ln, off):
    return 4 * int(ln) - (int(off) + 1).bit_length() + 1 if ln else -1000


def census(pre, blk, depth):
    """The serial LAZY2 parse over orc_deep_matches (as orc_lz_parse_deep walks them), counting the
    steps decided at the rule's exact margins, the takes of a capped match and the takes that end
    at or past lim.  Also returns the parse, which must be the oracle's own."""
    ln, off = oracle_matches(pre, blk, depth)
    nb = len(blk)
    lim = max(len(pre) + nb - HASH_READ, len(pre)) - len(pre)  # in block positions
    g = [gain(ln[i], off[i]) for i in range(nb)] + [-1000, -1000]
    c = dict(g1_take4=0, g1_defer5=0, g2_take7=0, g2_defer8=0, take64=0, take_to_lim=0)
    seqs, p, anchor = [], 0, 0
    while p < lim:
        if ln[p] == 0:
            p += 1
            continue
        d1, d2 = g[p + 1] - g[p], g[p + 2] - g[p]
        if d1 > 4 or d2 > 7:
            c["g1_defer5"] += d1 == 5
            c["g2_defer8"] += d2 == 8 and d1 <= 4
            p += 1
            continue
        c["g1_take4"] += d1 == 4
        c["g2_take7"] += d2 == 7
        c["take64"] += ln[p] == MAX_MATCH
        c["take_to_lim"] += p + ln[p] >= lim
        ll, of = p - anchor, int(off[p])
        if seqs and ll == 0 and seqs[-1][2] == of:
            seqs[-1][1] += int(ln[p])
        else:
            seqs.append([ll, int(ln[p]), of])
        p += int(ln[p])
        anchor = p
    return {k: int(v) for k, v in c.items()}, [tuple(s) for s in seqs]


def expected_literals(blk, seqs, last):
    out, pos = bytearray(), 0
    for ll, ml, _ in seqs:
        out += bytes(blk[pos:pos + ll])
        pos += ll + ml
    out += bytes(blk[pos:pos + last])
    return bytes(out)


# ---- the library's path function ------------------------------------------------------------------
_lib = None


def deep_lib():
    """The HIP library (its path function and split need no device)."""
    global _lib
    if _lib is None:
        import cuda_zstd

        _lib = cuda_zstd.lib()
    return _lib


def deep_path(pre, nb, s0=0):
    """(DEEP_PATH_*, segment length) of zh_test_deep_path."""
    segl = ctypes.c_uint32()
    f = deep_lib().zh_test_deep_path
    f.restype = ctypes.c_int
    p = f(ctypes.c_uint32(pre), ctypes.c_uint32(nb), ctypes.c_uint32(s0), ctypes.byref(segl))
    return p, segl.value


def deep_split(cn):
    """(staged content bytes P, split) of a dictionary of cn content bytes; (0, 0): no tables."""
    P, sp = ctypes.c_uint32(), ctypes.c_uint32()
    deep_lib().zh_test_deep_split(ctypes.c_uint64(cn), ctypes.byref(P), ctypes.byref(sp))
    return P.value, sp.value


def first_nb_off(pre, s0, path):
    """The smallest nb in [1, BLOCK] whose path is above `path` (None: there is none)."""
    lo, hi = 1, BLOCK + 1  # the path is monotone in nb
    while lo < hi:
        mid = (lo + hi) // 2
        if deep_path(pre, mid, s0)[0] > path:
            hi = mid
        else:
            lo = mid + 1
    return lo if lo <= BLOCK else None


# ---- case builders --------------------------------------------------------------------------------
def text(n, seed, kind=T.DG_TEXT):
    return T.gen(kind, 1, seed, n)


A_SIZES = (1, 2, 7, 8, 9, 12, 13, 63, 64, 65, 1023, 1024, 1025)


def cases_sizes():
    src = text(2048, 0xDEE90001)
    out = [(f"text{n}", EMPTY, src[:n].copy(), 0) for n in A_SIZES]
    out += [("rle1", EMPTY, np.array([7], np.uint8), 0), ("rle2", EMPTY, np.array([5, 5], np.uint8), 0)]
    for n in (2, 3, 9, 100, 4097):
        d = np.full(n, 0x61, np.uint8)
        d[-1] = 0x62
        out.append((f"const{n}_last_differs", EMPTY, d, 0))
    # a block that ends in zeros: past its end the slot is zero padded, so a match inside the run
    # goes on matching there, and only the cap at n - p ends it
    out.append(("text1000_then_zeros", EMPTY, np.concatenate([src[:1000], np.zeros(200, np.uint8)]), 0))
    out.append(("one_then_zeros", EMPTY, np.concatenate([np.array([1], np.uint8), np.zeros(300, np.uint8)]), 1))
    return out


def cases_thresholds():
    """(name, prefix, block, tables, expected path, expected segment length or None): every
    threshold of the path function from both sides.  The sizes come from the function itself."""
    out = []
    txt = text(2 * BLOCK, 0xDEE90002)
    js = text(2 * BLOCK, 0xDEE90003, T.DG_JSON)

    def add(nm, pre, nb, tables, path, segl=None, src=txt):
        out.append((nm, src[:pre].copy(), src[pre:pre + nb].copy(), tables, path, segl))

    a = first_nb_off(0, 0, DEMAND)
    b = first_nb_off(0, 0, LDS_BYTES)
    add("nopre_demand_last", 0, a - 1, 0, DEMAND, 32)
    add("nopre_demand_first_off", 0, a, 0, LDS_BYTES)
    add("nopre_bytes_last", 0, b - 1, 0, LDS_BYTES, None, js)
    add("nopre_bytes_first_off", 0, b, 0, LDS_LINKS, None, js)
    add("nopre_16384", 0, 16384, 0, DEMAND, 16)
    add("nopre_16385", 0, 16385, 0, DEMAND, 32)
    add("nopre_65536", 0, 65536, 0, LDS_LINKS)
    add("pre32k_nb32k", 32768, 32768, 0, LDS_LINKS, None, js)
    e = first_nb_off(DEEP_PRE, 0, LDS_LINKS)  # E = pre + nb - ZH_HASH_READ crosses what LDS holds
    add("pre64k_links_last", DEEP_PRE, e - 1, 0, LDS_LINKS)
    add("pre64k_links_first_off", DEEP_PRE, e, 0, SLOT)
    add("pre64k_nb64k", DEEP_PRE, 65536, 0, SLOT, None, js)
    s0 = deep_split(DEEP_PRE)[1]
    t = first_nb_off(DEEP_PRE, s0, DEMAND)
    add("dict64k_16384", DEEP_PRE, 16384, 1, DEMAND, 32, js)
    add("dict64k_16385", DEEP_PRE, 16385, 1, DEMAND, 64, js)
    add("dict64k_demand_last", DEEP_PRE, t - 1, 1, DEMAND, 64)
    add("dict64k_demand_first_off", DEEP_PRE, t, 1, LDS_BYTES)
    return out


C_OFFSETS, C_PRES, C_NBS = (0, 1, 4, 15), (0, 16, 17, 4104), (4096, 4097, 4111)


def cases_staging():
    src = text(16384, 0xDEE90004)
    return [(f"off{o}_pre{p}_nb{n}", src[:p].copy(), src[p:p + n].copy(), o) for o in C_OFFSETS for p in C_PRES for n in C_NBS]


def cases_slot_reuse():
    """Two runs for one slot (nslots = 1): a random 64 KiB block, then text blocks of 100, 1000 and
    5000 bytes; and 64 KiB of text, then its own first 100, 1000 and 5000 bytes, so the stale bytes
    past each short block are exactly the bytes that would lengthen its last matches."""
    rng = np.random.default_rng(0xDEE9)
    src = text(BLOCK, 0xDEE90005)
    other = text(8192, 0xDEE90006)
    a = [("random64k", EMPTY, rng.integers(0, 256, BLOCK, dtype=np.uint8), 0)] + [(f"then_text{n}", EMPTY, other[:n].copy(), 0) for n in (100, 1000, 5000)]
    b = [("text64k", EMPTY, src, 0)] + [(f"then_its_first{n}", EMPTY, src[:n].copy(), 0) for n in (100, 1000, 5000)]
    return a, b


D_PERIODS = (2, 3, 5, 63, 64, 65, 255, 256)


def cases_periodic():
    rng = np.random.default_rng(0xDEEA)
    out = []
    for p in D_PERIODS:
        unit = rng.permutation(256)[:p].astype(np.uint8)
        for n in (4096, 20000):
            out.append((f"period{p}_{n}", EMPTY, np.tile(unit, n // p + 1)[:n].copy(), 0))
    return out


# lim = n - ZH_HASH_READ at the chain rounds' boundaries and 256 +- 1 positions past a round start
D_LIMS = (255, 257, HB - 1, HB, HB + 1, HB + 255, HB + 256, HB + 257, 2 * HB + 1)


def cases_lims():
    src = text(2 * HB + 64, 0xDEE90007)
    return [(f"lim{lim}", EMPTY, src[:lim + HASH_READ].copy(), 0) for lim in D_LIMS]


D_DEPTHS = (4, 8, 16, 32, 64, 128)


DECOY = 8  # bytes per lone key: the key and three bytes that occur nowhere else in the key or tail


def decoy(k, seed=0xDEEB):
    """key + tail, k x (key + 3 other bytes), key + tail: the last key's chain holds the k lone keys
    (5-byte matches) before the first key + tail, so the 45-byte match is candidate k + 1.  The last
    key is at decoy_pos(k)."""
    rng = np.random.default_rng(seed)
    sym = rng.permutation(256).astype(np.uint8)
    key, tail, pad, rest = sym[:5], sym[5:45], sym[45:85], sym[85:]
    lone = [np.concatenate([key, rng.choice(rest, 3)]) for _ in range(k)]
    return np.concatenate([pad[:16], key, tail] + lone + [key, tail, pad[16:40]])


def decoy_pos(k):
    return 16 + 45 + DECOY * k


def cases_decoys(d):
    return [(f"decoy_depth{d}_k{k}", EMPTY, decoy(k), 0) for k in (d - 1, d)]


def cases_offset_bound():
    """A random 64 KiB prefix and a block that begins with prefix[k : k + 200]: offsets 65536 (no
    match), 65535 and 65534; and blocks whose match has a near candidate (10 bytes, in range) whose
    next link (20 bytes) is exactly 65535 / 65536 away."""
    rng = np.random.default_rng(0xDEEC)
    pre = rng.integers(0, 256, DEEP_PRE, dtype=np.uint8)
    out = [(f"offset{DEEP_PRE - k}", pre, np.concatenate([pre[k:k + 200], rng.integers(0, 256, 56, dtype=np.uint8)]), 0) for k in (0, 1, 2)]
    pre2 = pre.copy()
    x = rng.integers(0, 256, 20, dtype=np.uint8)
    pre2[100:120] = x
    pre2[40000:40010] = x[:10]
    for nm, at in (("near_then_65535", 99), ("near_then_65536", 100)):  # staged position 65536 + at, candidates 40000 and 100
        blk = rng.integers(0, 256, 400, dtype=np.uint8)
        blk[at:at + 20] = x
        out.append((nm, pre2, blk, 0))
    return out


# LAZY2 margins: 16 KiB of text whose serial parse decides at every margin at least once (the
# census; checked on the CPU by tests/test_deep_inputs.py).  (depth, generator seed)
E_INPUTS = ((4, 0xDEE90010), (32, 0xDEE90010))
E_PRE = 32768  # prefix (no tables) that moves the same blocks to a full-search path
E_FLOORS = ("g1_take4", "g1_defer5", "g2_take7", "g2_defer8")


def cases_lazy(depth, seed, with_prefix):
    src = text(E_PRE + 16384, seed)
    if with_prefix:
        return (f"lazy_d{depth}_pre", src[:E_PRE].copy(), src[E_PRE:].copy(), 0)
    return (f"lazy_d{depth}", EMPTY, src[E_PRE:].copy(), 0)


F_CONTENTS = (71, 72, 75, 76, 1000, 1021, 65536, 70000)


def cases_dict():
    """(name, content, block): JSON content of each length and a 4096-byte JSON block that repeats
    content bytes from below the split, from [split, pre), and a run that ends in the block's own
    first bytes (a match across the content / block boundary)."""
    out = []
    for cn in F_CONTENTS:
        content = text(cn, 0xDEE90020 + cn, T.DG_JSON)
        tail = content[-DEEP_PRE:]
        P = len(tail)
        blk = text(4096, 0xDEE90021, T.DG_JSON).copy()
        blk[500:540] = tail[10:50]  # below the split
        blk[1500:1516] = tail[P - 16:P]  # over the split, to the content's last byte
        blk[2500:2540] = np.concatenate([tail[P - 20:], blk[:20]])  # across the boundary
        out.append((f"content{cn}", content, blk))
    return out

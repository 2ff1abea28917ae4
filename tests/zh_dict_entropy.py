"""Helpers of tests/test_gpu_dict_entropy.py (test infrastructure): hand-built formatted
dictionaries (RFC 8878 section 5: direct-weights Huffman header, FSE table descriptions from
zh_seqframes.ncount_bytes, repcodes, content), the first sequence of a frame's first block, and
the three compression paths with CompressionConfig::dict_entropy."""
import numpy as np

import zh_seqframes as S
import zh_testlib as T

DICT_MAGIC = 0xEC30A437


def huf_direct(lengths):
    """Huffman tree description with direct 4-bit weights for {byte value: code length}: a complete
    prefix code whose highest byte value is <= 128.  Returns the header bytes."""
    last = max(lengths)
    log = max(lengths.values())
    assert last <= 128 and sum(1 << (log - l) for l in lengths.values()) == 1 << log
    w = [log + 1 - lengths[s] if s in lengths else 0 for s in range(last)]  # the last weight is implied
    if len(w) & 1:
        w.append(0)
    return bytes([127 + last]) + bytes((w[i] << 4) | w[i + 1] for i in range(0, len(w), 2))


def make_dict(content, huf, of=None, ml=None, ll=None, reps=(1, 4, 8), dict_id=0x12345):
    """Formatted dictionary: huf = {byte value: code length}; of / ml / ll = (normalised counts, log),
    default the predefined distributions."""
    ll, of, ml = ll or S.PREDEF[0], of or S.PREDEF[1], ml or S.PREDEF[2]
    out = DICT_MAGIC.to_bytes(4, "little") + dict_id.to_bytes(4, "little") + huf_direct(huf)
    for (norm, log), maxsv in ((of, 31), (ml, 52), (ll, 35)):
        out += S.ncount_bytes(list(norm), log, maxsv)
    out += b"".join(int(r).to_bytes(4, "little") for r in reps)
    return out + bytes(content)


def read_ncount(b):
    """FSE table description at b -> (normalised counts, log, bytes used)."""
    bits = int.from_bytes(b[:64], "little")
    log = (bits & 15) + 5
    pos, rem, thr, nb, norm, prev0 = 4, (1 << log) + 1, 1 << log, log + 1, [], False
    while rem > 1:
        if prev0:
            while True:
                r = (bits >> pos) & 3
                pos += 2
                norm += [0] * r
                if r != 3:
                    break
        mx = 2 * thr - 1 - rem
        v = (bits >> pos) & (thr - 1)
        if v < mx:
            pos += nb - 1
        else:
            v = (bits >> pos) & (2 * thr - 1)
            if v >= thr:
                v -= mx
            pos += nb
        c = v - 1
        rem -= abs(c)
        norm.append(c)
        prev0 = c == 0
        while rem < thr:
            nb -= 1
            thr >>= 1
    assert rem == 1
    return norm, log, (pos + 7) // 8


def dict_tables(d):
    """(LL, OF, ML) (normalised counts, log) of formatted dictionary d (its Huffman header skipped)."""
    o = 8
    hb = d[o]
    o += 1 + ((hb - 127 + 1) // 2 if hb >= 128 else hb)
    t = []
    for _ in range(3):
        norm, log, used = read_ncount(d[o:])
        t.append((norm, log))
        o += used
    return t[2], t[0], t[1]


def first_sequence(frame, dictionary):
    """(literal length code, offset value, match length code) of the first sequence of the frame's
    first block (a compressed block with sequences); offset values 1..3 are the repeat offsets.
    Only the three initial FSE states are read: they give the first sequence's codes."""
    b = bytes(frame)
    fhd = b[4]
    single, did, fcsf = (fhd >> 5) & 1, fhd & 3, fhd >> 6
    ip = 5 + (0 if single else 1) + (0, 1, 2, 4)[did] + ((1 if single else 0), 2, 4, 8)[fcsf]
    bh = int.from_bytes(b[ip:ip + 3], "little")
    assert (bh >> 1) & 3 == 2, "the first block is not a compressed block"
    blk = b[ip + 3:ip + 3 + (bh >> 3)]
    lt, sf = blk[0] & 3, (blk[0] >> 2) & 3
    if lt <= 1:
        lhs = (1, 2, 1, 3)[sf]
        n = blk[0] >> 3 if lhs == 1 else int.from_bytes(blk[:lhs], "little") >> 4
        p = lhs + (n if lt == 0 else 1)
    else:
        lhs = 3 if sf <= 1 else sf + 2
        nb = 10 if sf <= 1 else 14 if sf == 2 else 18
        p = lhs + ((int.from_bytes(blk[:lhs], "little") >> (4 + nb)) & ((1 << nb) - 1))
    nseq = blk[p]
    assert 0 < nseq < 128
    modes = blk[p + 1]
    p += 2
    dt = dict_tables(dictionary)
    tabs = []
    for t in range(3):  # LL, OF, ML
        m = (modes >> (6 - 2 * t)) & 3
        if m == 0:
            tabs.append(S.PREDEF[t])
        elif m == 1:
            tabs.append(blk[p])
            p += 1
        elif m == 2:
            norm, log, used = read_ncount(blk[p:])
            tabs.append((norm, log))
            p += used
        else:
            tabs.append(dt[t])
    bits = int.from_bytes(blk[p:], "little")
    pos = bits.bit_length() - 1  # the end mark
    codes = []
    for t in range(3):  # initial states: LL, OF, ML
        if isinstance(tabs[t], int):
            codes.append(tabs[t])
            continue
        norm, log = tabs[t]
        pos -= log
        codes.append(S.fse_cells(norm, log)[(bits >> pos) & ((1 << log) - 1)][0])
    ofc = codes[1]
    pos -= ofc
    return codes[0], (1 << ofc) + ((bits >> pos) & ((1 << ofc) - 1)), codes[2]


def dev(torch, b):
    a = np.frombuffer(bytes(b), np.uint8).copy()
    return torch.from_numpy(a if a.size else np.zeros(1, np.uint8)).cuda()[: len(a)]


def compress_paths(torch, recs, d, level, on):
    """The records as frames through Manager.compress, Manager.compress_batch and the batch manager
    (stream-ordered, device arrays): {path: [frame bytes]}."""
    import cuda_zstd

    dd = cuda_zstd.Dictionary.load(d)
    m = cuda_zstd.Manager(level, dict_entropy=on)
    m.set_dictionary(dd)
    dr = [dev(torch, r) for r in recs]
    out = {"compress": [m.compress(r).cpu().numpy().tobytes() for r in dr],
           "compress_batch": [f.cpu().numpy().tobytes() for f in m.compress_batch(dr)]}
    n, mx = len(recs), max(len(r) for r in recs)
    bc = cuda_zstd.BatchManager(level, mx, dict_entropy=on)
    bc.set_dictionary(dd)
    slot = (bc.max_out(mx) + 255) // 256 * 256
    ob = torch.empty(n * slot, dtype=torch.uint8, device="cuda")
    in_ptrs = torch.tensor([r.data_ptr() for r in dr], dtype=torch.int64, device="cuda")
    out_ptrs = ob.data_ptr() + torch.arange(n, dtype=torch.int64, device="cuda") * slot
    sizes = torch.tensor([len(r) for r in recs], dtype=torch.int64, device="cuda")
    osz = torch.zeros(n, dtype=torch.int64, device="cuda")
    st = torch.zeros(n, dtype=torch.int32, device="cuda")
    temp = torch.empty(bc.temp_size(n, mx), dtype=torch.uint8, device="cuda")
    bc.compress_async(in_ptrs, sizes, mx, out_ptrs, osz, st, temp)
    torch.cuda.synchronize()
    assert int((st != 0).sum()) == 0
    oh, sz = ob.cpu().numpy(), osz.cpu().numpy()
    out["batch_manager"] = [oh[i * slot:i * slot + int(sz[i])].tobytes() for i in range(n)]
    return out


def batch_total(torch, recs, d, level, on):
    """Total compressed bytes of the records through Manager.compress_batch, and the frames."""
    import cuda_zstd

    m = cuda_zstd.Manager(level, dict_entropy=on)
    m.set_dictionary(cuda_zstd.Dictionary.load(d))
    frames = [f.cpu().numpy().tobytes() for f in m.compress_batch([dev(torch, r) for r in recs])]
    return sum(len(f) for f in frames), frames

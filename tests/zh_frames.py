"""Header-level walker of RFC 8878 frames (test infrastructure): lists, per block, the
block type, literals-section type / header size / regenerated size / stream count / Huffman
weight encoding, the size of the sequence count and the three sequence-table modes, so the
tests can show which encoder and decoder paths a set of frames exercises.  Nothing is decoded;
a parse that is provably off (a reserved bit set, a section past its block, a frame that does
not end at the end of the buffer or at the next magic number) raises ValueError."""

LIT_TYPES = ("raw", "rle", "huffman", "treeless")
SEQ_MODES = ("predefined", "rle", "fse", "repeat")
RAW_RLE_HDR = (1, 2, 1, 3)  # Size_Format -> header bytes of raw / RLE literals (RFC 8878 §3.1.1.3.1.1)


def _need(b, ip, n, what):
    if ip + n > len(b):
        raise ValueError(f"{what} runs past the buffer")


def _literals(p, d):
    """Literals section at the start of block content p -> its size; fills d."""
    if not p:
        raise ValueError("empty compressed block")
    lt, sf = p[0] & 3, (p[0] >> 2) & 3
    d["lit"] = LIT_TYPES[lt]
    if lt <= 1:
        lhs = RAW_RLE_HDR[sf]
        if lhs > len(p):
            raise ValueError("literals header runs past the block")
        n = p[0] >> 3 if lhs == 1 else (int.from_bytes(p[:lhs], "little") >> 4)
        sec = lhs + (n if lt == 0 else 1)
    else:
        lhs = 3 if sf <= 1 else sf + 2
        if lhs > len(p):
            raise ValueError("literals header runs past the block")
        h = int.from_bytes(p[:lhs], "little")
        nb = 10 if sf <= 1 else 14 if sf == 2 else 18
        n = (h >> 4) & ((1 << nb) - 1)
        cs = (h >> (4 + nb)) & ((1 << nb) - 1)
        d["streams"] = 1 if sf == 0 else 4
        sec = lhs + cs
        if lt == 2:
            if cs < 1 or sec > len(p):
                raise ValueError("Huffman literals run past the block")
            d["weights"] = "fse" if p[lhs] < 128 else "direct"
    if sec > len(p):
        raise ValueError("literals section runs past the block")
    d["lit_hdr"], d["lit_n"] = lhs, n
    return sec


def _sequences(s, d):
    """Sequences section header s (the rest of the block after the literals); fills d."""
    if not s:
        raise ValueError("no sequences section")
    b0 = s[0]
    k = 1 if b0 < 128 else 2 if b0 < 255 else 3
    if k > len(s):
        raise ValueError("sequence count runs past the block")
    d["nseq_bytes"] = k
    d["nseq"] = b0 if k == 1 else (((b0 - 128) << 8) + s[1] if k == 2 else s[1] + (s[2] << 8) + 0x7F00)
    if d["nseq"] == 0:
        if len(s) != k:  # (libzstd: srcSize_wrong)
            raise ValueError("bytes after an empty sequences section")
        return
    if k >= len(s):
        raise ValueError("sequence modes run past the block")
    m = s[k]
    if m & 3:
        raise ValueError("reserved bits of the sequence modes are set")
    d["modes"] = (SEQ_MODES[m >> 6], SEQ_MODES[(m >> 4) & 3], SEQ_MODES[(m >> 2) & 3])
    # one byte per RLE table, at least one per FSE table description, one of bitstream
    if k + 1 + sum(1 for x in d["modes"] if x in ("rle", "fse")) + 1 > len(s):
        raise ValueError("sequence tables run past the block")


def walk(frame: bytes):
    """-> list of per-block dicts; raises ValueError on a malformed header."""
    b = bytes(frame)
    ip, blocks = 0, []
    while ip < len(b):
        _need(b, ip, 4, "magic")
        magic = int.from_bytes(b[ip:ip + 4], "little")
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            _need(b, ip, 8, "skippable frame header")
            ip += 8 + int.from_bytes(b[ip + 4:ip + 8], "little")
            if ip > len(b):
                raise ValueError("skippable frame runs past the buffer")
            blocks.append({"type": "skippable"})
            continue
        if magic != 0xFD2FB528:
            raise ValueError("bad magic")
        _need(b, ip, 5, "frame header")
        fhd = b[ip + 4]
        single, chk, did, fcsf = (fhd >> 5) & 1, (fhd >> 2) & 1, fhd & 3, fhd >> 6
        if fhd & 8:
            raise ValueError("reserved bit of the frame header descriptor is set")
        hs = 1 + (0 if single else 1) + (0, 1, 2, 4)[did] + ((1 if single else 0), 2, 4, 8)[fcsf]
        _need(b, ip, 4 + hs, "frame header")
        dp = ip + 5 + (0 if single else 1)
        dict_id = int.from_bytes(b[dp:dp + (0, 1, 2, 4)[did]], "little")
        ip += 4 + hs
        first = True
        while True:
            _need(b, ip, 3, "block header")
            bh = int.from_bytes(b[ip:ip + 3], "little")
            last, bt, bsz = bh & 1, (bh >> 1) & 3, bh >> 3
            ip += 3
            d = {"type": ("raw", "rle", "compressed", "reserved")[bt], "size": bsz, "first_in_frame": first, "checksum": bool(chk),
                 "single_segment": bool(single), "fcs": fcsf != 0 or bool(single), "dict_id": dict_id}
            first = False
            if bt == 3:
                raise ValueError("reserved block type")
            n = 1 if bt == 1 else bsz
            _need(b, ip, n, "block")
            if bt == 2:
                p = b[ip:ip + bsz]
                _sequences(p[_literals(p, d):], d)
            ip += n
            blocks.append(d)
            if last:
                break
        if chk:
            _need(b, ip, 4, "checksum")
            ip += 4
    return blocks


def features(frames):
    """Set of encoder / decoder paths the frames exercise."""
    f = set()
    for fr in frames:
        for d in walk(fr):
            f.add("block_" + d["type"])
            if d.get("checksum"):
                f.add("checksum")
            if not d.get("fcs", True):
                f.add("no_fcs")
            if "single_segment" in d and not d["single_segment"]:
                f.add("window_descriptor")
            if d["type"] == "compressed":
                f.add("lit_" + d["lit"])
                f.add(f"lit_{'huf' if d['lit'] == 'huffman' else d['lit']}_h{d['lit_hdr']}")
                if "streams" in d:
                    f.add(f"huf_{d['streams']}stream")
                if "weights" in d:
                    f.add("weights_" + d["weights"])
                    f.add(f"huf_{d['streams']}stream_weights_{d['weights']}")
                f.add(f"nseq_bytes{d['nseq_bytes']}")
                if d["nseq"] == 0:
                    f.add("no_sequences")
                for t, m in zip(("ll", "of", "ml"), d.get("modes", ())):
                    f.add(f"{t}_{m}")
    return f

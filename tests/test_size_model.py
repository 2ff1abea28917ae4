"""The size pass's plain-Python model (tests/zh_size_model.py) against known truth, on the CPU: the
hand-assembled sequence vectors (zh_seqframes), the committed libzstd frames
(tests/golden/decode_frames.json, with frames that state no content size, Repeat_Mode tables and
treeless literals among them), hand-made concatenations whose size is the sum of their parts, and
truncated buffers.  tests/test_gpu_decompress_size.py holds zh_dec_size_kernel to this model."""
import json
import os

import zh_frames as F
import zh_seqframes as S
import zh_size_model as M
import zh_testlib as T


def _s_form_cut(v):
    """v's bytes cut one byte short of the end of its last block."""
    tail = 4 if v.buf[-1].get("checksum") else 0
    return v.bytes[:len(v.bytes) - tail - 1]


def test_sequence_vectors():
    """Every accepted vector's size is its decoded length; of the rejected ones the model rejects
    what the sequence reader can see and sizes what only an execution can (a bad offset)."""
    seen = set()
    for v in S.vectors():
        size, ok = M.size(v.bytes)
        if v.expect == "nonzero":  # a Dictionary_ID no dictionary answers
            assert not ok, v
        elif v.want is not None:
            assert ok and size == len(v.want), v
            # the model's block walk and zh_frames.walk agree on what the blocks are
            assert sum(1 for d in F.walk(v.bytes) if d["type"] != "skippable") == sum(len(f["blocks"]) for f in v.buf if "blocks" in f), v
        else:
            seen.add((v.name, ok))
            fcs = all(f["fcs"] for f in v.buf if "blocks" in f)
            blind = v.name.startswith("bad_offset")
            assert ok == (fcs or blind), (v, ok)
            if ok:
                assert size == sum(S._claimed_size(f) for f in v.buf if "blocks" in f), v
    # both verdicts occur among the rejected vectors: the model is not trivially permissive
    assert {ok for _, ok in seen} == {True, False}, seen


def test_rejects_without_fcs():
    """The defects the sequence reader sees, in frames without a content size (whatever header
    rotation the vectors have): each is rejected; the same frame with a content size is sized."""
    cases = {"ll_exceeds_literals": S._block("ll_exceeds_literals", [(5, 4, 4), (6, 3, 5)], lits=b"0123456789"),
             "regen_131073": S._block("regen_131073", [(10, 131063, 6)]),
             "surplus_byte": S._block("surplus_byte", S.PRE + S.READ, 2, surplus=True),
             "last_byte_zero": S._block("last_byte_zero", S.PRE + S.READ, 2, zero_last=True)}
    for name, blk in cases.items():
        for pre in ([], [S.raw(S.PRE_RAW)]):
            assert M.size(S.assemble([S.frame(pre + [blk], fcs=False)])) == (0, False), name
            claimed = len(S.PRE_RAW) * len(pre) + S._claimed_size(S.frame([blk]))
            assert M.size(S.assemble([S.frame(pre + [blk], fcs=True)])) == (claimed, True), name
    ok_blk = S._block("fine", S.PRE + S.READ, 2)
    assert M.size(S.assemble([S.frame([ok_blk], fcs=False)])) == (S._claimed_size(S.frame([ok_blk])), True)


def test_dictionary_vectors():
    d = S.dictionary()
    for v in S.dict_vectors():
        size, ok = M.size(v.bytes, d)
        if v.want is not None:
            assert ok and size == len(v.want), v
        else:  # an offset past the dictionary: not the size pass's to see
            assert ok and size == S._claimed_size(v.buf[0]), v


def test_golden_decode_frames():
    vecs = json.load(open(os.path.join(T.GOLDEN, "decode_frames.json")))["vectors"]
    names = {v["name"] for v in vecs}
    assert "exe_10k_l3_nofcs" in names
    summed = 0
    for v in vecs:
        frame = bytes.fromhex(v["frame"])
        size, ok = M.size(frame)
        if "expect_error" in v:
            continue
        assert ok and size == v["size"], v["name"]
        summed += any(not b.get("fcs", True) for b in F.walk(frame))
    assert summed >= 1


def test_golden_frames_summed_when_the_content_size_is_dropped():
    """Every golden frame re-framed without its Frame_Content_Size (the blocks unchanged): the sum
    over the blocks is the recorded length, for every entropy path the fixture set reaches."""
    vecs = json.load(open(os.path.join(T.GOLDEN, "decode_frames.json")))["vectors"]
    frames = []
    for v in vecs:
        if "expect_error" in v:
            continue
        frame = M.drop_content_size(bytes.fromhex(v["frame"]))
        if frame is None:
            continue
        assert M.size(frame) == (v["size"], True), v["name"]
        frames.append(frame)
    assert len(frames) >= 20
    assert F.features(frames) >= {"no_fcs", "ll_repeat", "of_repeat", "ml_repeat", "lit_treeless", "ll_rle", "of_fse", "ml_fse", "nseq_bytes2",
                                  "no_sequences", "block_raw", "block_rle"}


def test_hand_made_sums():
    for name, data, want, _ in M.hand_made():
        assert M.size(data) == (want, True), name
    assert any(want >= M.FCS_2_40 for _, _, want, _ in M.hand_made())


def test_overflow_and_empty():
    big = [d for name, d, _, _ in M.hand_made() if name == "fcs_2_40"][0]
    top = big[:5] + ((1 << 64) - 2).to_bytes(8, "little") + big[13:]
    assert M.size(top) == ((1 << 64) - 2, True)
    assert M.size(top + top) == (0, False)  # the sum leaves 64 bits
    assert M.size(b"") == (0, False)


def test_truncation():
    n = 0
    for v in S.vectors():
        if v.form != "S" or v.expect == "nonzero":
            continue
        assert M.size(_s_form_cut(v)) == (0, False), v
        n += 1
    assert n > 50
    for v in S.vectors()[:8]:
        for cut in range(1, 7):  # inside the frame header, or before the first block header ends
            assert M.size(v.bytes[:cut]) == (0, False), (v, cut)
    for name, data, _, _ in M.hand_made():
        assert M.size(data[:-1]) == (0, False), name


def test_formatted_dictionary_tables():
    """A frame without a content size whose first block repeats a formatted dictionary's tables:
    sized with the dictionary, rejected without it (nothing to repeat / Dictionary_ID)."""
    import zh_dict_entropy as DE

    content = S._rng("size_dict").integers(0, 256, 4096, dtype="uint8").tobytes()
    of = S._fse_norm([2, 3], 5)[1:]
    ml = S._fse_norm([2, 6], 7)[1:]
    ll = S._fse_norm([4, 9], 6)[1:]
    d = DE.make_dict(content, {65: 1, 66: 2, 67: 2}, of=of, ml=ml, ll=ll, dict_id=0x4242)
    seqs = [(4, 5, 6), (9, 9, 9)]
    blk = S._block("size_dict_blk", seqs, 1, modes=("repeat",) * 3)
    # the assembler needs tables to repeat from: a first block sets them, then the frame is cut to the second
    prev = [S.Table(S.fse_cells(list(n), lg), lg) for n, lg in (ll, of, ml)]
    body = S._block_bytes(blk, True, prev)
    want = S._claimed_size(S.frame([blk]))
    for did_bytes, fhd in ((b"", 0x00), ((0x4242).to_bytes(2, "little"), 0x02)):
        frame = S.MAGIC.to_bytes(4, "little") + bytes([fhd, 0x00]) + did_bytes + body
        assert M.size(frame, d) == (want, True)
        assert M.size(frame) == (0, False)

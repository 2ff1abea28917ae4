"""Hand-assembled Huffman literals vectors on the CPU (no GPU): the vectors of tests/zh_hufframes.py
reach every named state of the decoder's segment-parallel stream decode (zh_decode.hip,
huf_streams_par) with 64 segments (one stream) and with 16 (four streams), which the segment tracer
-- a plain restatement of that scheme that reads the emitted bytes alone -- makes a checked fact;
the tracer accepts and rejects what the model does, and libzstd decodes every vector to the model's
bytes and rejects what the model rejects.  The GPU test (test_gpu_decode_literals.py) decodes the
same vectors."""
import hashlib

import pytest

import zh_frames as F
import zh_hufframes as H
import zh_seqframes as S
import zh_testlib as T


def test_sequence_vectors_unchanged():
    """The assembler learnt Huffman literals; the existing vectors keep their bytes (digests taken
    with the assembler as it was before)."""
    want = {"v": (189, "734ddbb9658c0573bbc47e2a047c5633875a675de8752b2dbeb0e17f406b5d84"),
            "d": (20, "6e865070ed7491d36118da30ceba08ebbdc9288b8ad2838ff82e304d3a69ea6c")}
    for key, vs in (("v", S.vectors()), ("d", S.dict_vectors())):
        h = hashlib.sha256()
        for v in vs:
            h.update(repr(v).encode() + len(v.bytes).to_bytes(4, "little") + v.bytes)
        assert (len(vs), h.hexdigest()) == want[key]


@pytest.mark.parametrize("streams", [1, 4])
def test_vectors_reach_every_segment_state(streams):
    """Every tag of the tracer is reached by a valid vector, with 64 segments and with 16.  No tag
    proved unreachable: a merge past the 32 recorded positions with 64 segments, where a one-stream
    section's 1,023 symbols average 16 a segment, takes a code whose 11-bit symbols stretch the
    segments around a run of 2- and 4-bit ones (slow_long_1s, found with the tracer)."""
    have = set()
    for v in H.vectors():
        if v.want is not None:
            have |= H.vector_trace(v)[1][streams]
    assert have >= set(H.TAGS), sorted(set(H.TAGS) - have)


def test_named_vectors_have_their_states():
    """The vectors chosen for one state have it (a change of data or n that loses it fails here)."""
    by = {v.name: H.vector_trace(v)[1] for v in H.vectors() if v.form == "Q" or v.name.startswith("treeless")}
    one, four = (lambda n: by[n][1]), (lambda n: by[n][4])  # noqa: E731
    assert {"Lb1", "empty_segments", "zero_symbols", "no_fixup"} <= one("two_syms_0")
    assert all("Lb1" in one(f"two_syms_{n}") for n in list(range(10)) + [63, 64]) and "Lb1" not in one("two_syms_65")
    assert "empty_segments" not in one("two_syms_64") and "empty_segments" in one("two_syms_65")
    assert "rounds_max" in one("fixed7_1000") and "no_fixup" in one("fixed7_1023")
    assert "rounds_max" in one("fixed8_256_1s") and "left_segment" in one("fixed8_256_1s")
    assert "merge_unrecorded" in one("slow_long_1s") and "below_bit0" in one("skew11_1023")
    for n in (3, 6, 9):
        assert {"zero_symbols", "Lb1", "empty_segments"} <= four(f"two_syms_4s_{n}")
    for name in ("fixed7_4s_rmax", "fixed8_256_4s_rmax", "even_4s_rmax"):
        assert {"rounds_max", "left_segment"} <= four(name), name
    assert "merge_unrecorded" in four("slow_4s_3000") and "no_fixup" in four("two_syms_4s_131072")


def test_tracer_verdict_equals_model():
    for v in H.vectors():
        ok, _ = H.vector_trace(v)  # (also: accepted sections decode to the description's bytes)
        assert ok == (v.want is not None), v


def test_libzstd_decodes_every_vector_to_the_model(libzstd):
    """No vector is skipped.  libzstd returns the model's bytes for every valid vector and an error
    for every reject (the rejects carry no checksum and no content size, so the error is for the
    defect).  One version difference: newer libzstd rejects a 4-stream section of fewer than 6
    literals, 1.4.9 (the version the oracle restates) and zh_decode.hip decode it; for those two
    vectors libzstd may return the model's bytes or an error."""
    may = set()
    for v in H.vectors():
        if v.want is None:
            assert not any(f.get("checksum") or f.get("fcs") for f in v.buf), v
            with pytest.raises(AssertionError):
                T.zstd_decompress(v.bytes, v.cap + 65536)
            continue
        if v.opts.get("libzstd_may_reject"):
            may.add(v.name)
            try:
                got = T.zstd_decompress(v.bytes, len(v.want))
            except AssertionError:
                continue
            assert got == v.want, v
            continue
        assert T.zstd_decompress(v.bytes, len(v.want)) == v.want, v
        if v.expect == S.TOO_SMALL:
            with pytest.raises(AssertionError):
                T.zstd_decompress(v.bytes, v.cap)
    assert may == {"two_syms_4s_3", "two_syms_4s_4"}


def test_model_rejects():
    assert {v.name for v in H.vectors() if v.want is None} == H.REJECTED
    assert all(v.expect == S.CORRUPT for v in H.vectors() if v.want is None)
    assert [v.name for v in H.vectors() if v.expect == S.TOO_SMALL] == ["cap_short_4s"]
    # the table state is the frame's: a tree, then treeless sections, are the description's bytes
    a, b = bytes(range(7)) * 9, bytes([6, 5, 4, 3, 2, 1, 0]) * 5
    two = [S.comp(H.huf(a, H.EVEN), []), S.comp(H.huf(b, H.EVEN, 4, tree=False), [])]
    assert S.model([S.frame(two)])[0] == a + b
    assert S.model([S.frame(two[1:])])[0] is None and S.model([S.frame(two), S.frame(two[1:])])[0] is None


def test_stream_rejects_fail_the_intended_check():
    """A stream's verdict has two arms.  The short-code vectors pass the first (the segment counts add
    up to the symbol count: zero fill below bit 0 finds the right last symbol) and fail only the
    second (the last exit is below bit 0): a reader that clamps its position at 0 accepts them.  A
    Regenerated_Size that is off, or a zero byte in front, fails the count."""
    why = {}
    for v in H.vectors():
        if v.want is None:
            t = H.vector_trace(v)[1]
            why[v.name] = (t[1] | t[4]) & {"bad_count", "bad_exit"}
    assert why["short_code"] == why["short_code_4s"] == {"bad_exit"}
    for name in ("regen_plus1", "regen_minus1", "regen4_minus1", "regen4_plus3", "zero_front", "zero_front_4s"):
        assert why[name] == {"bad_count"}, name
    assert why["boundary_moved"] and not why["zero_last"] and not why["zero_append"]  # (no final bit flag: no stream to trace)


def test_walker_sees_the_intended_sections():
    """zh_frames.walk reports, for each Huffman or treeless block, the literals type, header size,
    stream count and weight encoding the vector was written to have."""
    seen = set()
    for v in H.vectors():
        blocks = [b for b in F.walk(v.bytes) if b["type"] == "compressed" and b["lit"] in ("huffman", "treeless")]
        got = [(b["lit"], b["lit_hdr"], b["streams"], b.get("weights")) for b in blocks]
        assert got == v.opts["walk"], v
        if v.want is not None:
            seen |= set(got)
            assert [b["lit_n"] for b in blocks] == [len(h["data"]) for h in H.huf_blocks(v)], v
    # all four Size_Formats, both weight encodings with 1 and with 4 streams, treeless both ways
    assert seen >= {("huffman", 3, 1, "direct"), ("huffman", 3, 1, "fse"), ("huffman", 3, 4, "direct"), ("huffman", 4, 4, "direct"),
                    ("huffman", 4, 4, "fse"), ("huffman", 5, 4, "direct"), ("treeless", 3, 1, None), ("treeless", 3, 4, None),
                    ("treeless", 4, 4, None)}


def test_descriptions_are_what_they_claim():
    by = {v.name: v for v in H.vectors() if v.form in "Q"}
    sec = lambda name: H.huf_blocks(by[name])[0]["_sec"]  # noqa: E731
    assert sec("two_syms_1")[3] == 128 and sec("fixed7_1000")[3] == 127 + 127 and sec("even_1s")[3] == 127 + 6
    assert sec("direct_even_1s")[3:5] == bytes([127 + 2, 0x21])
    assert H.code_table(H.TWO_SYMS)[0] == 1 and H.code_table(H.SKEW11)[0] == 11
    assert sorted(k for _, k in H.code_table(H.SKEW11)[1].values()) == list(range(1, 12)) + [11]
    assert sorted(k for _, k in H.code_table(H.EVEN)[1].values()) == [2, 2, 2, 4, 4, 4, 4]
    # FSE-compressed weights: 255 of them (state 1 ends the stream) and 254 (state 2 does)
    for name, nw in (("fixed8_256_1s", 255), ("fixed8_255_1s", 254), ("spread_1s", 255)):
        s = sec(name)
        assert s[3] < 128 and len(H.read_weights(s[3:])[0]) == nw + 1, name
    assert {s // 64 for s in H.SPREAD_SYMS} == {0, 1, 2, 3} and len(set(H.SPREAD)) == 6
    # 9 literals in 4 streams: the fourth stream is the single byte 01; Compressed_Size at its end
    assert sec("two_syms_4s_9")[-1:] == b"\x01" and H.stream_counts(9, 4) == [3, 3, 3, 0]
    assert len(sec("skew11_1023")) == 3 + 1023
    assert len(by["two_syms_4s_131072"].want) == S.BLOCK_MAX
    assert [v.name for v in H.vectors() if v.align16] == ["fixed7_1000", "skew11_4s_1021", "even_4s_1023", "fixed7_4s_rmax"]
    for name in ("skew11_4s_1021", "even_4s_1023", "fixed7_4s_rmax"):  # stream sizes of both parities, an odd one first
        s = sec(name)
        at = 4 + 1 + (s[4] - 127 + 1) // 2 if sec(name)[0] >> 2 & 3 == 2 else 3 + 1 + (s[3] - 127 + 1) // 2
        sizes = [int.from_bytes(s[at + 2 * i:at + 2 * i + 2], "little") for i in range(3)]
        assert any(x & 1 for x in sizes), (name, sizes)


def test_vector_budget():
    vs = H.vectors()
    assert len({v.bytes for v in vs}) == len(vs) <= 160
    assert sum(len(v.want) for v in vs if v.want is not None) < 8 << 20
    assert max(len(v.bytes) for v in vs) <= 128 * 1024 and max(v.cap for v in vs) <= 128 * 1024 + 16

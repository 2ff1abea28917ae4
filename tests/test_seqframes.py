"""Hand-assembled sequence vectors on the CPU (no GPU): the vectors of tests/zh_seqframes.py
reach every named case of the sequence semantics (repeat offsets, overlap periods, window edges,
sequence counts, length / offset codes, bits per step, table shapes, dictionary sources) in both
forms -- the block as its buffer's only block (Q: the decoder's quad sequence kernel) and after
a 1-byte raw block (S: its serial reader) -- and libzstd decodes every one of them to the model's
bytes and rejects what the model rejects (but for two documented version differences).  The GPU test (test_gpu_decode_sequences.py) decodes
the same vectors."""
import pytest

import zh_frames as F
import zh_seqframes as S
import zh_testlib as T


def _tags(vs, form):
    return set().union(*[v.tags for v in vs if v.form == form and v.expect == 0])


@pytest.mark.parametrize("form", ["Q", "S"])
def test_vectors_cover_every_sequence_path(form):
    have = _tags(S.vectors(), form)
    need = S.ALL_SEQ_PATHS | (S.S_ONLY_SEQ_PATHS if form == "S" else set())
    assert have >= need, sorted(need - have)
    have = _tags(S.dict_vectors(), form)
    assert have >= S.DICT_SEQ_PATHS, sorted(S.DICT_SEQ_PATHS - have)


def test_forms_take_the_intended_decoder_path():
    """Q: the buffer ends with its one frame's only block (what zh_decode.hip hands to the quad
    kernel); S: the compressed blocks are never a buffer's first and last block."""
    for v in S.vectors() + S.dict_vectors():
        blocks = [b for b in F.walk(v.bytes) if b["type"] != "skippable"]
        comp = [b for b in blocks if b["type"] == "compressed"]
        assert comp, v
        if v.form == "Q":
            assert len(blocks) == 1, v
        else:
            assert len(blocks) > 1, v
    names = {}
    for v in S.vectors() + S.dict_vectors():
        names.setdefault(v.name, set()).add(v.form)
    one_form = {n for n, f in names.items() if f != {"Q", "S"}}
    # what cannot be a buffer's only block (a second block or frame, megabytes of history), and
    # the Dictionary_ID frame
    assert one_form == {"first_rep3_ll0", "history_across_blocks", "history_reset_frame2", "of_codes_high", "repeat_after_predefined",
                        "repeat_after_rle", "repeat_after_fse", "bad_offset_later_block", "dict_id_without_dictionary"}


def test_vector_budget():
    vs = S.vectors() + S.dict_vectors()
    # (the issue's estimate was roughly 150 frames and 16 MiB: the 31 one-per-offset overlap frames,
    # each in two forms, are 62 frames and 7.75 MiB of it)
    assert len({v.bytes for v in vs}) == len(vs) <= 210
    assert sum(len(v.want) for v in vs if v.want is not None) < 20 << 20


def test_libzstd_decodes_every_vector_to_the_model(libzstd):
    """No vector is skipped.  libzstd returns the model's bytes for every valid vector and an error
    for every reject, but for two rejects where its versions differ and zh_decode.hip follows
    RFC 8878; there it gives an error or exactly the bytes of the same frame with the defect ignored:
    - regen_131073, the block that regenerates 131,073 bytes (RFC 8878 3.1.1.2.4 forbids more than
      128 KiB).  libzstd 1.4.9 (the version the oracle restates) accepts it in form Q and
      in form S and returns the 131,073 (131,074) bytes; zh_decode.hip rejects it.
    - surplus_byte, a sequence bitstream with one byte the sequences do not consume (RFC 8878,
      sequence decoding: a bitstream not entirely consumed after the last sequence is corrupted).
      libzstd 1.4.9 does not check this after the last sequence and returns the
      frame's bytes, at every stream length tried (1 to 1,000 sequences); zh_decode.hip rejects it.
    The rejects carry no content checksum, so the error is for the defect itself."""
    for v in S.vectors() + S.dict_vectors():
        if v.want is None or v.expect == "nonzero":
            assert not any(f.get("checksum") for f in v.buf), v
            try:
                got = T.zstd_decompress(v.bytes, v.cap + 65536, dictionary=v.dictionary)
            except AssertionError:
                continue
            assert v.libzstd_may_return is not None and got == v.libzstd_may_return, f"{v}: libzstd accepts what the model rejects"
            continue
        assert T.zstd_decompress(v.bytes, len(v.want), dictionary=v.dictionary) == v.want, v
        if v.expect == S.TOO_SMALL:
            with pytest.raises(AssertionError):
                T.zstd_decompress(v.bytes, v.cap, dictionary=v.dictionary)


def test_model_rejects():
    bad = {v.name for v in S.vectors() + S.dict_vectors() if v.want is None}
    assert bad == {"bad_offset_first", "bad_offset_later_block", "dict_bad_offset", "ll_exceeds_literals", "regen_131073", "surplus_byte",
                   "last_byte_zero"}
    # repeat history (RFC 8878 3.1.1.5): 1, 4, 8 at a frame start; value 3 with no literals is rep0 - 1, 0 forced to 1
    out, tags, _ = S.model([S.frame([S.comp(b"abcdefgh", [(8, 3, 1), (0, 4, 3)])])])
    assert out == b"abcdefgh" + b"hhh" + b"hhhh" and "rep3_ll0_forced_to_1" in tags
    out, _, _ = S.model([S.frame([S.comp(b"abcdefghij", [(8, 3, 2), (1, 3, 3), (1, 3, 3)])])])
    assert out == b"abcdefgh" + b"efg" + b"i" + b"efg" + b"j" + b"jjj"  # offsets 4, 8, then the old rep0 = 1

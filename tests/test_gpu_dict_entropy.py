"""CompressionConfig::dict_entropy on the GPU (Dictionaries): with a formatted
dictionary the first block of a frame starts from the dictionary's repcodes and may reuse its
Huffman table (treeless literals) and FSE tables (Repeat_Mode).  The oracle has no such path, so
the frames are checked by libzstd's decoder, by both GPU decode paths and by the header walker;
with the switch off the frames are the oracle's."""
import numpy as np
import pytest

import zh_dict_entropy as D
import zh_frames as F
import zh_seqframes as S
import zh_testlib as T

pytestmark = pytest.mark.gpu

SIZES = [1, 5, 6, 62, 63, 255, 256, 1024, 4096, 32768, 32769, 70000]
LEVELS = [1, 2, 3, 9]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def zdict():
    a = T.gen(T.DG_JSON, 512, 0x5EED0005, 4096)  # the ZDICT dictionary of test_gpu_dict.py's fixture
    return T.zdict_train([a[i:i + 4096] for i in range(0, len(a), 4096)], 16384)


def _records(n, size, seed=0x5EED0905):
    a = T.gen(T.DG_JSON, n, seed, size)
    return [a[i * size:(i + 1) * size] for i in range(n)]


def _mgr(d, level=3, on=True):
    import cuda_zstd

    m = cuda_zstd.Manager(level, dict_entropy=on)
    m.set_dictionary(cuda_zstd.Dictionary.load(d))
    return m


def _one(torch, m, data):
    return m.compress(D.dev(torch, data)).cpu().numpy().tobytes()


def _reused(blk):
    return blk.get("lit") == "treeless" or "repeat" in blk.get("modes", ())


def _check_decodes(torch, m, frames, recs, d):
    """libzstd and Manager.decompress on every frame."""
    for f, r in zip(frames, recs):
        want = bytes(r)
        assert T.zstd_decompress(f, len(want), dictionary=d) == want
        assert m.decompress(D.dev(torch, f), len(want)).cpu().numpy().tobytes() == want


def test_round_trip_every_path(torch_cuda, zdict):
    """Records of every size class at levels 1, 2, 3 and 9 through compress, compress_batch and the
    batch manager with the switch on: libzstd and Manager.decompress decode every frame, every
    frame names the dictionary, only first blocks reuse the dictionary's tables; then all frames
    together (over 2,048 buffers) through decompress_batch, the decoder's split pipeline."""
    src = T.gen(T.DG_JSON, 1, 0x5EED0A05, 70000)
    recs = [src[:n] for n in SIZES]
    did = T.dict_layout(zdict)[0]
    all_frames, all_want = [], []
    for level in LEVELS:
        m = _mgr(zdict, level)
        paths = D.compress_paths(torch_cuda, recs, zdict, level, True)
        assert paths["compress"] == paths["compress_batch"], level
        for name, frames in paths.items():
            _check_decodes(torch_cuda, m, frames, recs, zdict)
            for f, r in zip(frames, recs):
                blocks = F.walk(f)
                assert all(b["dict_id"] == did for b in blocks), (level, name, len(r))
                assert not any(_reused(b) for b in blocks[1:]), (level, name, len(r))
                assert len(blocks) > 1 or len(r) <= 65536
            all_frames += frames
            all_want += [bytes(r) for r in recs]
    m = _mgr(zdict, 3)
    k = (2048 + len(all_frames) - 1) // len(all_frames)
    frames, want = all_frames * k, all_want * k
    flat = D.dev(torch_cuda, b"".join(frames))
    offs = np.concatenate([[0], np.cumsum([len(f) for f in frames])])
    outs, st = m.decompress_batch([flat[offs[i]:offs[i + 1]] for i in range(len(frames))], [len(w) for w in want], raise_on_error=False)
    assert st == [0] * len(frames)
    for k, (o, w) in enumerate(zip(outs[:len(all_frames)], all_want)):
        assert o.cpu().numpy().tobytes() == w, k
    assert all(o.numel() == len(w) for o, w in zip(outs, want))


@pytest.fixture(scope="module")
def totals(torch_cuda, zdict):
    """{(record size, level, switch): (total compressed bytes, frames)} over 256 records."""
    out = {}
    for size in (512, 1024):
        recs = _records(256, size)
        for level in (3, 9):
            for on in (False, True):
                out[size, level, on] = D.batch_total(torch_cuda, recs, zdict, level, on)
    return out


def test_paths_are_reached(torch_cuda, zdict, totals):
    """256 records of 1 KiB at level 3: treeless literals and Repeat_Mode in each of the three
    positions occur in first blocks with the switch on, never with it off, and the frames with
    the switch off are the oracle's."""
    recs = _records(256, 1024)
    on = [F.walk(f)[0] for f in totals[1024, 3, True][1]]
    off = [F.walk(f)[0] for f in totals[1024, 3, False][1]]
    assert any(b.get("lit") == "treeless" for b in on)
    for t in range(3):
        assert any(b.get("modes", ("",) * 3)[t] == "repeat" for b in on), t
    assert not any(_reused(b) for b in off)
    for f, r in zip(totals[1024, 3, False][1], recs):
        assert f == T.oracle_frame(r, dictionary=zdict)
    m = _mgr(zdict)
    _check_decodes(torch_cuda, m, totals[1024, 3, True][1][:32], recs[:32], zdict)


@pytest.mark.parametrize("level", [3, 9])
@pytest.mark.parametrize("size", [512, 1024])
def test_it_pays(totals, size, level):
    """The dictionary's tables make small records smaller: strictly fewer total bytes with the switch
    on (libzstd gains 10-18 % on these shapes; tools/dict_entropy_bench.py measures ours)."""
    on, off = totals[size, level, True][0], totals[size, level, False][0]
    print(f"{size} B x 256, level {level}: {off} -> {on} bytes ({100.0 * (on - off) / off:+.1f} %)")
    assert on < off


# ---- hand-built dictionaries: the encoder must refuse a table that cannot code the block -------
HUF16 = {v: 4 for v in range(97, 113)}   # 'a'..'p', 4 bits each
HUF64 = {v: 6 for v in range(32, 96)}    # 64 byte values, 6 bits each


def _rng(seed):
    return np.random.default_rng(seed)


def _content(seed, n, lo, hi):
    return _rng(seed).integers(lo, hi, n, dtype=np.uint8).tobytes()


def _first(frame):
    return F.walk(frame)[0]


def test_refuses_uncovered_literals(torch_cuda):
    """(a) a Huffman table with codes for 16 byte values: a record of those values gets treeless
    literals, the same record with one other byte value does not."""
    d = D.make_dict(_content(1, 1024, 128, 256), HUF16)
    m = _mgr(d)
    rec = bytearray(_rng(2).integers(97, 113, 200, dtype=np.uint8).tobytes())
    f = _one(torch_cuda, m, rec)
    assert _first(f)["lit"] == "treeless"
    _check_decodes(torch_cuda, m, [f], [rec], d)
    rec[77] = ord("z")
    f = _one(torch_cuda, m, rec)
    assert _first(f)["type"] == "raw" or _first(f)["lit"] != "treeless"
    _check_decodes(torch_cuda, m, [f], [rec], d)


def test_refuses_offset_table_without_the_code(torch_cuda):
    """(b) an offset table with probability for codes <= 10 only: a match 4 KiB back must not use
    Repeat_Mode for offsets, near matches do."""
    content = _content(3, 4096, 0, 256)
    d = D.make_dict(content, HUF64, of=([3] * 10 + [2], 5))
    m = _mgr(d)
    tail = _content(4, 24, 0, 256)
    far = content[:64] + tail
    f = _one(torch_cuda, m, far)
    b = _first(f)
    assert b["type"] == "compressed" and b["modes"][1] != "repeat"
    _check_decodes(torch_cuda, m, [f], [far], d)
    near = content[-100:-36] + tail[:8] + content[-400:-340] + tail[8:16] + content[-900:-840] + tail
    f = _one(torch_cuda, m, near)
    b = _first(f)
    assert b["type"] == "compressed" and b["modes"][1] == "repeat"
    _check_decodes(torch_cuda, m, [f], [near], d)


def test_refuses_length_tables_without_the_code(torch_cuda):
    """(c) literal-length and match-length tables each missing a code the record needs (literal
    length 0, the code of a 64-byte match): neither table is repeated."""
    content = _content(5, 4096, 0, 256)
    ll = list(S.LL_NORM)
    ll[1] += ll[0]
    ll[0] = 0
    ml = list(S.ML_NORM)
    c = S.ml_code(64)
    ml[0] += ml[c]
    ml[c] = 0
    d = D.make_dict(content, HUF64, ll=(ll, 6), ml=(ml, 6))
    m = _mgr(d)
    rec = content[-300:-236] + _content(6, 24, 0, 256)
    f = _one(torch_cuda, m, rec)
    b = _first(f)
    assert b["type"] == "compressed"
    llc, _, mlc = D.first_sequence(f, d)
    assert (llc, mlc) == (0, c)
    assert b["modes"][0] != "repeat" and b["modes"][2] != "repeat"
    _check_decodes(torch_cuda, m, [f], [rec], d)


def test_no_sequences_rle_and_random(torch_cuda):
    """(d) 64 distinct covered bytes: treeless literals and no sequences; (e) one repeated byte is
    still an RLE block; (f) random bytes are still a raw block."""
    d = D.make_dict(_content(7, 1024, 128, 256), HUF64)
    m = _mgr(d)
    perm = _rng(8).permutation(np.arange(32, 96, dtype=np.uint8)).tobytes()
    f = _one(torch_cuda, m, perm)
    b = _first(f)
    assert b["type"] == "compressed" and b["lit"] == "treeless" and b["nseq"] == 0
    run, rnd = b"A" * 300, _content(9, 300, 0, 256)
    fr, fn = _one(torch_cuda, m, run), _one(torch_cuda, m, rnd)
    assert _first(fr)["type"] == "rle" and _first(fn)["type"] == "raw"
    _check_decodes(torch_cuda, m, [f, fr, fn], [perm, run, rnd], d)


def test_dictionary_repcodes(torch_cuda):
    """A dictionary with repcodes 7 / 300 / 4000 over 4 KiB of content: a record that opens with
    three literals and then repeats with period 7 codes its first offset as repeat offset 1; a
    record that copies from 300 back at position 0 (literal length 0, where the repeat offsets
    shift by one) codes it as offset value 1 too.  With the switch off both are real offsets."""
    content = _content(10, 4096, 0, 256)
    d = D.make_dict(content, HUF64, reps=(7, 300, 4000))
    rec = bytearray(_content(11, 3, 0, 256))
    while len(rec) < 35:
        rec.append(rec[-7] if len(rec) >= 7 else content[len(rec) - 7])
    rec7 = bytes(rec) + _content(12, 16, 0, 256)
    rec300 = content[-300:-260] + _content(13, 16, 0, 256)
    m, m0 = _mgr(d), _mgr(d, on=False)
    f7, f300 = _one(torch_cuda, m, rec7), _one(torch_cuda, m, rec300)
    assert D.first_sequence(f7, d)[1] == 1
    llc, ofv, _ = D.first_sequence(f300, d)
    assert (llc, ofv) == (0, 1)
    assert D.first_sequence(_one(torch_cuda, m0, rec7), d)[1] == 7 + 3
    assert D.first_sequence(_one(torch_cuda, m0, rec300), d)[1] == 300 + 3
    _check_decodes(torch_cuda, m, [f7, f300], [rec7, rec300], d)


def test_switch_needs_a_formatted_dictionary(torch_cuda, zdict):
    """The switch changes nothing without a dictionary or with raw content."""
    import cuda_zstd

    rec = _records(1, 1024)[0]
    content = zdict[T.dict_layout(zdict)[1]:]
    for d in (None, content):
        out = []
        for on in (False, True):
            m = cuda_zstd.Manager(3, dict_entropy=on)
            if d:
                m.set_dictionary(cuda_zstd.Dictionary.load(d))
            out.append(_one(torch_cuda, m, rec))
        assert out[0] == out[1] == T.oracle_frame(rec, dictionary=d)


# ---- finalisation: raw content + the samples' statistics -> a formatted dictionary --------------
def test_finalize(torch_cuda):
    """64 samples of 512 B over 4 KiB of trained content: the result parses (ID >= 32768 by libzstd's
    hash rule, the content unchanged), libzstd compresses and decompresses with it, two calls and
    device / host samples give equal bytes, one 8-byte sample is enough, an explicit ID is kept."""
    import cuda_zstd

    recs = _records(65, 512, 0x5EED0B05)
    samples = [r.tobytes() for r in recs[:64]]
    raw = cuda_zstd.Dictionary.train(samples, 4096)
    content = raw.content()
    fd = raw.finalize(samples).content()
    did, off = T.dict_layout(fd)
    assert did == S.xxh64(content) % (2 ** 31 - 32768) + 32768 and did >= 32768
    assert fd[off:] == content and fd[:4] == D.DICT_MAGIC.to_bytes(4, "little")
    rec = recs[64].tobytes()
    assert T.zstd_decompress(T.zstd_compress_dict(rec, fd, 3), len(rec), dictionary=fd) == rec
    assert raw.finalize(samples).content() == fd
    assert raw.finalize([D.dev(torch_cuda, s) for s in samples]).content() == fd
    assert raw.finalize(D.dev(torch_cuda, b"".join(samples)).view(64, 512)).content() == fd
    assert cuda_zstd.Dictionary.train(samples, 4096, finalize=True).content() == fd
    one = raw.finalize([b"8 bytes!"]).content()
    assert T.dict_layout(one)[1] > 0 and one[T.dict_layout(one)[1]:] == content
    assert T.zstd_decompress(T.zstd_compress_dict(rec, one, 3), len(rec), dictionary=one) == rec
    assert T.dict_layout(raw.finalize(samples, dict_id=424242).content())[0] == 424242
    l9 = raw.finalize(samples, level=9).content()
    assert l9[T.dict_layout(l9)[1]:] == content


def test_train_finalize_compress_end_to_end(torch_cuda):
    """Train on half of 512 records of 1 KiB, finalise, compress the other half with the switch on:
    fewer total bytes than the same records against the raw content, and libzstd decodes them."""
    import cuda_zstd

    recs = _records(512, 1024, 0x5EED0C05)
    train, test = [r.tobytes() for r in recs[0::2]], recs[1::2]
    raw = cuda_zstd.Dictionary.train(train, 16384)
    fd = raw.finalize(train).content()
    t_raw, _ = D.batch_total(torch_cuda, test, raw.content(), 3, True)
    t_fd, frames = D.batch_total(torch_cuda, test, fd, 3, True)
    print(f"256 x 1 KiB, level 3: raw content {t_raw} -> finalised {t_fd} bytes ({100.0 * (t_fd - t_raw) / t_raw:+.1f} %)")
    assert t_fd < t_raw
    _check_decodes(torch_cuda, _mgr(fd), frames[:32], test[:32], fd)

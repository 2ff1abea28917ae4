"""GPU decoder (zh_decode.hip), Huffman literals by construction: the hand-assembled vectors of
tests/zh_hufframes.py (test_hufframes.py shows which states of the segment-parallel stream decode
they reach, and that libzstd decodes them to the same bytes) decoded on the MI355X, bytes and status
against the plain model: huf_read_weights with direct and FSE-compressed descriptions at their
limits, huf_build_dtable over all four lane groups, huf_streams_par with 64 and with 16 segments,
treeless sections, every reject of the section.  A batch of 2,304 buffers takes the split pipeline
(the tables pass defers the blocks that have sequences, the rest pass decodes their literals)."""
import pytest

import zh_hufframes as H
import zh_seqframes as S
from test_gpu_decode_sequences import _arena, _entries, _mgr, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def test_literal_vectors(torch_cuda):
    """All vectors in one batch: the one-pass walker; the Q forms that have sequences go through
    the quad sequence kernel and the execution kernel.  A 4-stream section of 3 or 4 literals is
    accepted (as libzstd 1.4.9 does; DESIGN.md, decoder)."""
    n = _run(torch_cuda, _mgr(), H.vectors())
    assert len(H.vectors()) + 4 * 15 == n < 1024


def test_literal_vectors_split_pipeline(torch_cuda):
    """The set repeated cyclically to 2,304 buffers (4.8 MiB of output)."""
    assert _run(torch_cuda, _mgr(), H.vectors(), 2304) == 2304


def test_stream_alignments(torch_cuda):
    """The align16 vectors (one stream; four streams with odd stream sizes) with their first byte at
    each of the 16 alignments: stream starts and ends at every byte of a dword."""
    vs = [v for v in H.vectors() if v.align16]
    assert len(vs) == 4 and sorted({h["streams"] for v in vs for h in H.huf_blocks(v)}) == [1, 4]
    entries = _entries(vs)
    keep, frames = _arena(torch_cuda, entries)
    assert sorted({f.data_ptr() % 16 for f in frames}) == list(range(16))
    assert _run(torch_cuda, _mgr(), vs) == 64


def test_size_query_reads_every_size_format(torch_cuda):
    """Manager.decompressed_sizes over every valid vector framed without a content size: the
    Regenerated_Size of Huffman and treeless sections at all four Size_Formats (literals_regen)."""
    torch = torch_cuda
    vs = [v for v in H.vectors() if v.want is not None]
    bufs = [H.without_content_size(v) for v in vs]
    assert {hdr for v in vs for _, hdr, _, _ in v.opts["walk"]} == {3, 4, 5}
    assert {(h["_sec"][0] >> 2) & 3 for v in vs for h in H.huf_blocks(v)} == {0, 1, 2, 3}
    import numpy as np

    dev = [torch.from_numpy(np.frombuffer(b, np.uint8).copy()).cuda() for b in bufs]
    sizes, st = _mgr().decompressed_sizes(dev, raise_on_error=False)
    bad = [(repr(v), s, c, len(v.want)) for v, s, c in zip(vs, sizes, st) if c != 0 or s != len(v.want)]
    assert not bad, bad[:12]
    assert S.BLOCK_MAX in sizes and 0 in sizes

"""Many streams in one call (cuda_zstd_stream_batch_*; zh_window_update_kernel, csrc/zh_stream.hip):
six streams whose windows stay on the device, compressed and decoded one chunk per stream per round.

The schedules cover a growing window, a sliding one (len + n > 64 KiB with n < 64 KiB), a replaced one
(n = 65,536, 65,537 and 200,000), n = 1, an idle round, and chunk tensors at offsets 1, 3, 7 and 15."""
import functools

import numpy as np
import pytest

import zh_testlib as T

pytestmark = pytest.mark.gpu

MAX_CHUNK = 200000
W = 65536
SCHEDULES = [  # chunk bytes per round, one row per stream (0: idle)
    [10000, 30000, 20000, 9000],      # grow, then slide by a little
    [50000, 30000, 1, 40000],         # slide: 50,000 + 30,000 > 64 KiB
    [1000, 65536, 65537, 200000],     # replace
    [40000, 1, 1, 30000],             # n = 1
    [20000, 0, 30000, 5],             # an idle round in the middle
    [65535, 1, 65536, 100],           # one byte short of full, filled, replaced
]
OFFSETS = [1, 3, 7, 15]
ROUNDS = 4


@functools.lru_cache(maxsize=None)
def streams():
    return [T.gen(T.DG_JSON if i % 2 == 0 else T.DG_TEXT, 1, 0x5EED0D00 + i, sum(s)) for i, s in enumerate(SCHEDULES)]


def schedule():
    """Per round: [(chunk, history) or None per stream], history = the stream's last <= 64 KiB."""
    pos = [0] * len(SCHEDULES)
    rounds = []
    for r in range(ROUNDS):
        row = []
        for i, s in enumerate(streams()):
            n = SCHEDULES[i][r]
            if n == 0:
                row.append(None)
                continue
            row.append((s[pos[i]:pos[i] + n], s[max(0, pos[i] - W):pos[i]]))
            pos[i] += n
        rounds.append(row)
    return rounds


def device_chunk(c, off):
    """The chunk as a device tensor that starts `off` bytes into its allocation."""
    import torch

    host = np.zeros(off + len(c), np.uint8)
    host[off:] = c
    t = torch.from_numpy(host).cuda()[off:]
    assert t.data_ptr() % 16 == off
    return t


@pytest.mark.parametrize("level", [3, 9])
def test_streams(libzstd, level):
    import torch

    import cuda_zstd

    ns = len(SCHEDULES)
    sb = cuda_zstd.StreamBatch(level, ns, MAX_CHUNK)
    singles = [cuda_zstd.StreamingManager(level) for _ in range(ns)]
    all_frames = []
    for r, row in enumerate(schedule()):
        chunks = [None if it is None else device_chunk(it[0], OFFSETS[(i + r) % 4]) for i, it in enumerate(row)]
        frames, st = sb.compress_chunks(chunks)
        torch.cuda.synchronize()
        host = []
        for i, it in enumerate(row):
            if it is None:  # idle: status 2, size 0
                assert st[i] == 2 and frames[i] is None, (r, i)
                host.append(None)
                continue
            c, h = it
            f = frames[i].cpu().numpy().tobytes()
            assert st[i] == 0
            assert f == T.oracle_frame(c, dictionary=h.tobytes() if len(h) else None, level=level), (r, i, len(c), len(h))
            one = singles[i].compress_chunk(chunks[i], with_history=True).cpu().numpy().tobytes()
            assert f == one, (r, i, "StreamingManager")
            host.append(f)
        all_frames.append(host)
    # the decoding direction: every stream in order, frames at odd offsets too
    for r, (row, host) in enumerate(zip(schedule(), all_frames)):
        fr = [None if f is None else device_chunk(np.frombuffer(f, np.uint8), OFFSETS[(i + r + 1) % 4]) for i, f in enumerate(host)]
        back, st = sb.decompress_chunks(fr)
        torch.cuda.synchronize()
        for i, it in enumerate(row):
            if it is None:
                assert st[i] != 0 and back[i] is None, (r, i)
            else:
                assert st[i] == 0 and back[i].cpu().numpy().tobytes() == it[0].tobytes(), (r, i)
    # after reset the first frames are dictionary-less again, in both directions
    sb.reset()
    row = schedule()[0]
    frames, st = sb.compress_chunks([device_chunk(it[0], 1) for it in row])
    torch.cuda.synchronize()
    assert st == [0] * ns
    plain = [f.cpu().numpy().tobytes() for f in frames]
    assert plain == [T.oracle_frame(it[0], level=level) for it in row]
    back, st = sb.decompress_chunks(frames)
    assert st == [0] * ns and [b.cpu().numpy().tobytes() for b in back] == [it[0].tobytes() for it in row]
    sb.close()


def test_failed_stream_keeps_its_window(libzstd):
    """A stream whose frame does not decode keeps its decoded window: the next good frame still
    decodes behind it; its neighbour is untouched."""
    import torch

    import cuda_zstd

    s = streams()[0]
    a, b = s[:20000], s[20000:45000]
    sb = cuda_zstd.StreamBatch(3, 2, MAX_CHUNK)
    f0, st = sb.compress_chunks([device_chunk(a, 1), device_chunk(a, 3)])
    f1, st1 = sb.compress_chunks([device_chunk(b, 7), device_chunk(b, 15)])
    assert st == [0, 0] == st1
    assert f1[0].cpu().numpy().tobytes() == T.oracle_frame(b, dictionary=a.tobytes(), level=3)
    back, st = sb.decompress_chunks(f0)
    assert st == [0, 0]
    bad = f1[0].clone()
    bad[:4] = 0  # no magic
    back, st = sb.decompress_chunks([bad, f1[1]])
    assert st[0] != 0 and back[0] is None and st[1] == 0 and back[1].cpu().numpy().tobytes() == b.tobytes()
    back, st = sb.decompress_chunks([f1[0], None])
    assert st[0] == 0 and back[0].cpu().numpy().tobytes() == b.tobytes() and st[1] != 0
    with pytest.raises(cuda_zstd.ZstdError):
        cuda_zstd.StreamBatch(3, 0, MAX_CHUNK)
    torch.cuda.synchronize()
    sb.close()

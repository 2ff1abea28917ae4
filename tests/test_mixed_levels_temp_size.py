"""Workspace size of the per-chunk-level batched compress entry (no GPU needed):
nvcomp_zstd_batched_compress_levels_get_temp_size_v5 covers what a dictionary-less handle at any
level needs for nvcomp_zstd_batched_compress_async_v5 with the same arguments, and grows with the
chunk count."""
import pytest

SHAPES = [(1, 1), (16, 65536), (16384, 65536), (8, 163840)]


@pytest.fixture(scope="module")
def L():
    import cuda_zstd

    return cuda_zstd.lib()


@pytest.mark.parametrize("n,m", SHAPES)
def test_covers_every_single_level_handle(L, n, m):
    need = L.nvcomp_zstd_batched_compress_levels_get_temp_size_v5(n, m)
    assert need > 0
    for level in range(1, 23):
        h = L.nvcomp_zstd_batch_create_v5(level, 65536, 0)
        assert h
        own = L.nvcomp_zstd_batch_get_batched_temp_size_v5(h, n, m)
        L.nvcomp_zstd_batch_destroy_v5(h)
        assert 0 < own <= need, (level, own, need)


def test_non_decreasing_in_the_chunk_count(L):
    for m in (1, 65536, 163840):
        sizes = [L.nvcomp_zstd_batched_compress_levels_get_temp_size_v5(n, m) for n in (1, 2, 3, 15, 16, 17, 255, 256, 257, 1000, 16384, 16385)]
        assert sizes == sorted(sizes), (m, sizes)

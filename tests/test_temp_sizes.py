"""Public compress temp sizes do not move (no GPU needed): callers allocate from these numbers, so
every dictionary-less size entry returns exactly the bytes recorded in tests/golden/temp_sizes.json
(tools/record_temp_sizes.py wrote it from the library before the workspace layout became one
function of one shape)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_every_dictionaryless_entry_returns_the_recorded_bytes():
    import cuda_zstd
    import record_temp_sizes as R

    with open(R.OUT) as f:
        want = json.load(f)
    got = R.sizes_of(cuda_zstd.lib())
    assert set(got) == {"batch_workspace", "batched_temp", "batch_compress_temp", "levels_temp", "single", "single_ldm"}
    for entry, sizes in got.items():
        assert sizes == want[entry], entry
    # the cases the record covers, so that an emptied golden file cannot pass
    assert sorted(map(int, got["single"])) == [1, 3, 4, 5, 9, 22]
    assert len(got["levels_temp"]) == 7 and all(len(v) == 5 for v in got["single_ldm"].values())
    assert all(v > 0 for v in got["levels_temp"].values())


def test_every_decode_entry_returns_the_recorded_bytes():
    """The decode-side queries at counts 1, 2 and 2,049 and capacities 1, 63, 64, 65, 131,072 and
    131,073.  dec_batched_temp, seek_read_temp and seek_ranges_temp follow the capacity across the
    decoder slot's 64-byte floor and 128 KiB cap; dec_single, dec_batch_workspace and dec_batch_temp
    size for 128 KiB blocks whatever the capacity."""
    import cuda_zstd
    import record_temp_sizes as R

    with open(R.OUT) as f:
        want = json.load(f)
    got = R.decode_sizes_of(cuda_zstd.lib())
    assert set(got) == {"dec_single", "dec_batch_workspace", "dec_batch_temp", "dec_batched_temp", "seek_read_temp", "seek_ranges_temp"}
    shapes = sorted(f"{n}x{c}" for n in (1, 2, 2049) for c in (1, 63, 64, 65, 131072, 131073))
    for entry, sizes in got.items():
        assert sizes == want[entry], entry
        assert sorted(sizes) == (shapes if entry != "dec_single" else sorted(map(str, (1, 63, 64, 65, 131072, 131073)))), entry
        assert all(v > 0 for v in sizes.values()), entry
    # the capacity-following entries: 1 and 64 bytes share the 64-byte floor, 128 KiB needs more than 65
    # bytes, and the decoder's own slots stop growing at the 128 KiB cap (the seekable reads' bounce
    # slots, sized by the frame, do not)
    for entry in ("dec_batched_temp", "seek_read_temp", "seek_ranges_temp"):
        assert got[entry]["1x1"] == got[entry]["1x64"] and got[entry]["1x65"] < got[entry]["1x131072"] <= got[entry]["1x131073"], entry
    assert got["dec_batched_temp"]["1x131072"] == got["dec_batched_temp"]["1x131073"]

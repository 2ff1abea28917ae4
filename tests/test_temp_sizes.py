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

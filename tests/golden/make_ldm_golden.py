"""Writes tests/golden/ldm_blocks.json from the numpy model (tests/zh_ldm_model.py): one-sequence
blocks, and the hash / sample predicate / slot / tag of every position of a 4 KiB buffer.
tests/cpp/ldm_block_check.cpp compares csrc/zh_ldm.h against it.  Flat strings, so the C++ side
needs no JSON library."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zh_ldm_model as M  # noqa: E402

TABLE_LOG = 13


def main():
    dists = sorted({d for c in range(15, 28) for d in ((1 << c) - 3, (1 << (c + 1)) - 4)} | {32769, 100000, (1 << 27) - 5, M.MAX_DIST})
    bases = [b for b, _ in M.ML_TABLE if b <= M.MIN_SEG + 3]
    mls = sorted({3, 34, M.MIN_SEG, M.MIN_SEG - 1, M.MIN_SEG + 1, 32768, 32767} | set(bases) | {b - 1 for b in bases})
    blocks = [f"{ml} {d} {last} {M.ldm_block(ml, d, last).hex()}" for d in dists for ml in mls for last in (0, 1)]
    rng = np.random.default_rng(0x1D3)
    buf = rng.integers(0, 256, 4096, dtype=np.uint8)
    buf[1000:1400] = 7  # a constant stretch
    buf[2000:2600] = buf[300:900]  # a repeat
    h = M.hashes(buf)
    assert len(h) == 4096 - 63 and M.hash_at(buf, 4032) == int(h[-1]) and M.hash_at(buf, 5) == int(h[5])
    out = {
        "table_log": str(TABLE_LOG),
        "blocks": ";".join(blocks),
        "buffer": buf.tobytes().hex(),
        "hashes": "".join(f"{int(v):016x}" for v in h),
        "samples": "".join("1" if s else "0" for s in M.is_sample(h)),
        "slots": "".join(f"{int(v):04x}" for v in M.slot_of(h, TABLE_LOG)),
        "tags": "".join(f"{int(v):08x}" for v in M.tag_of(h)),
        "table_logs": ";".join(f"{n} {hl} {M.table_log(n, hl)}" for n in (65537, 1 << 17, (1 << 17) + 1, 1 << 20, 1 << 24, (1 << 32) - 1) for hl in (10, 14, 20, 30)),
    }
    with open(os.path.join(HERE, "ldm_blocks.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print(len(blocks), "blocks,", len(h), "positions,", int(M.is_sample(h).sum()), "samples")


if __name__ == "__main__":
    main()

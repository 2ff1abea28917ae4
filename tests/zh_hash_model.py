"""The match finders' position hashes in numpy (csrc/zh_hash.h, include/zstd_hip_params.h), shared
by the tests that build inputs or expected tables from them."""
import os
import re

import numpy as np


def _params():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "zstd_hip_params.h")).read()
    names = r"ZH_HK_[LS]\d|ZH_HASH_LOG_LONG|ZH_HASH_LOG_SHORT|ZH_HASH_READ|ZH_DEEP_PRE|ZH_WINDOW|ZH_TILE"
    return {k: int(v, 0) for k, v in re.findall(r"#define (%s)\s+(\w+?)u?\s" % names, txt)}


P = _params()


def _le(b, lo, n):
    v = np.zeros(b.shape[:-1], dtype=np.uint64)
    for k in range(n):
        v |= b[..., lo + k].astype(np.uint64) << np.uint64(8 * k)
    return v


def hash_long(b):
    """The long table's slot of the 8 bytes b[..., 0:8] (include/zstd_hip_params.h)."""
    t = _le(b, 0, 3) * np.uint64(P["ZH_HK_L0"]) + _le(b, 3, 3) * np.uint64(P["ZH_HK_L1"]) + _le(b, 6, 2) * np.uint64(P["ZH_HK_L2"])
    return (t & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - P["ZH_HASH_LOG_LONG"])


def hash_short(b):
    """The short table's slot of the 5 bytes b[..., 0:5]."""
    t = _le(b, 0, 3) * np.uint64(P["ZH_HK_S0"]) + _le(b, 3, 2) * np.uint64(P["ZH_HK_S1"])
    return (t & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - P["ZH_HASH_LOG_SHORT"])

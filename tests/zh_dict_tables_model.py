"""Host model of a dictionary's precomputed tables, vectorised numpy: what the device builders
(zh_dict_hash_batch_kernel / zh_dict_pack_batch_kernel, zh_deep_dict_batch_kernel) must leave for a
dictionary's content bytes, written from the tables' definitions and sharing no code with them.

K1's tables: P = min(cn, 65535) (none if P < 2 * DTAB_MARGIN), tail = the last P content bytes,
B = P - DTAB_MARGIN; slot hash_long(tail[j:j+8]) of the long table and slot hash_short(tail[j:j+5])
of the short one hold the largest j + 1 over j < B, else 0; packed as u16, the long table first.

The deep matcher's chains: dP = min(cn, ZH_DEEP_PRE), split = (dP - ZH_HASH_READ) & ~3 (none if
split < 64); over the last dP content bytes prev[p], p < split, is 1 + the latest q < p with p's
short hash, else 0, and head[h] is 1 + the latest p < split hashing to h, else 0."""
import numpy as np

from zh_hash_model import P as PARAMS
from zh_hash_model import hash_long, hash_short

DTAB_MARGIN = 256  # csrc/zh_common.h ZH_DTAB_MARGIN
HL_SIZE, HS_SIZE = 1 << PARAMS["ZH_HASH_LOG_LONG"], 1 << PARAMS["ZH_HASH_LOG_SHORT"]
DEEP_PRE, HASH_READ = PARAMS["ZH_DEEP_PRE"], PARAMS["ZH_HASH_READ"]


def k1_shape(cn):
    """P for cn content bytes (0: no tables)."""
    p = min(cn, 65535)
    return p if p >= 2 * DTAB_MARGIN else 0


def deep_shape(cn):
    """(dP, split) for cn content bytes ((0, 0): no chains)."""
    dp = min(cn, DEEP_PRE)
    split = max(dp - HASH_READ, 0) & ~3
    return (dp, split) if split >= 64 else (0, 0)


def _latest(slots, size):
    """table[s] = 1 + the last index whose slot is s, else 0."""
    t = np.zeros(size, np.uint32)
    np.maximum.at(t, slots.astype(np.int64), np.arange(1, len(slots) + 1, dtype=np.uint32))
    return t


def k1_tables(content):
    """(P, the packed u16 tables) of the content bytes (a uint8 array); (0, None): none."""
    p = k1_shape(len(content))
    if not p:
        return 0, None
    win = np.lib.stride_tricks.sliding_window_view(content[len(content) - p:], 8)[:p - DTAB_MARGIN]
    return p, np.concatenate([_latest(hash_long(win), HL_SIZE), _latest(hash_short(win), HS_SIZE)]).astype(np.uint16)


def deep_chains(content):
    """(dP, split, prev[:split], head) of the content bytes; (0, 0, None, None): none."""
    dp, split = deep_shape(len(content))
    if not dp:
        return 0, 0, None, None
    h = hash_short(np.lib.stride_tricks.sliding_window_view(content[len(content) - dp:], 5)[:split])
    order = np.argsort(h, kind="stable")  # equal hashes stay in position order: neighbours are chain links
    same = h[order[1:]] == h[order[:-1]]
    prev = np.zeros(split, np.uint32)
    prev[order[1:][same]] = order[:-1][same] + 1
    return dp, split, prev, _latest(h, HS_SIZE)

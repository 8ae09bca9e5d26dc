"""Numpy restatement of remove_ids / update_index: what the compaction kernels (csrc/compact.hip) and plan_update
(wise_amd/index/mutate.py) must return.  Nothing here is shared with the code under test."""
import numpy as np


def bitmap(mask: np.ndarray) -> np.ndarray:
    """uint32 words of a boolean mask over row positions: bit (p & 31) of word p >> 5, tail bits zero."""
    n = mask.shape[0]
    bits = np.zeros((n + 31) // 32 * 32, dtype=np.uint8)
    bits[:n] = mask
    return np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view(np.uint32).copy()


def compact(a: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """The kept rows of `a` (first dimension = row) in their order."""
    return a[np.asarray(mask, dtype=bool)]


def rank(mask: np.ndarray, pos) -> np.ndarray:
    """Kept rows strictly before each position in [0, N]."""
    before = np.concatenate([[0], np.cumsum(np.asarray(mask, dtype=np.int64))])
    return before[np.asarray(pos, dtype=np.int64)]


def new_list_off(list_off: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """list_off [nlist + 1] after the rows with mask False are gone."""
    return rank(mask, list_off)


def plan_update(index_ids, store_ids):
    """(ids to remove, ascending; bool mask over store_ids of the rows to add) by sets."""
    have, want = set(int(i) for i in index_ids), set(int(i) for i in store_ids)
    remove = np.array(sorted(have - want), dtype=np.int64)
    add = np.array([int(i) not in have for i in store_ids], dtype=bool)
    return remove, add

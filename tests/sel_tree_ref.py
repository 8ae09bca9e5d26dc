"""numpy restatement of the selector trees (wise_amd/index/selector.py, csrc/sel_tree.hip) that the tests hold the kernels and the
recursion to.  A test helper: imported by tests only, never by wise_amd/.

  mask        a selector or a tree of selectors -> the boolean mask by row position, over (row ids, id_base, gid, group_keys)
  words       a mask as the uint32 words every bitmap entry point writes: bit (p & 31) of word p >> 5, the tail cleared
  combine     wise_sel_combine on words, the tail cleared whatever the inputs' tails hold
  groups_mask / idbits_mask   the two leaf rules on their own, as the C entry points state them
"""
import numpy as np

from wise_amd.index import selector as S


def row_ids(ids, id_base, n):
    """[n] int64: the external id of every row — ids, or id_base + row where ids is None"""
    return np.arange(n, dtype=np.int64) + int(id_base) if ids is None else np.asarray(ids, dtype=np.int64).reshape(-1)


def groups_mask(gid, group_keys, sel_keys):
    """[N] bool: 0 <= gid[p] < G and group_keys[gid[p]] occurs in sel_keys (any order, duplicates allowed)"""
    gid = np.asarray(gid, dtype=np.int64)
    group_keys = np.asarray(group_keys, dtype=np.int64)
    ok = (gid >= 0) & (gid < group_keys.size)
    out = np.zeros(gid.size, dtype=bool)
    out[ok] = np.isin(group_keys[gid[ok]], np.asarray(sel_keys, dtype=np.int64))
    return out


def idbits_mask(ids_of_rows, bits):
    """[N] bool: id i is selected iff i >= 0, i >> 3 < len(bits) and bit (i & 7) of bits[i >> 3] is set"""
    i = np.asarray(ids_of_rows, dtype=np.int64)
    bits = np.asarray(bits, dtype=np.uint8).reshape(-1)
    ok = (i >= 0) & ((i >> 3) < bits.size)
    out = np.zeros(i.size, dtype=bool)
    out[ok] = (bits[i[ok] >> 3] >> (i[ok] & 7).astype(np.uint8)) & 1 == 1
    return out


def mask(sel, ids, id_base, n, gid=None, group_keys=None):
    """[n] bool of any selector class or tree; gid / group_keys: the group tables (needed where the tree holds a group selector)"""
    rid = row_ids(ids, id_base, n)
    rec = lambda s: mask(s, ids, id_base, n, gid, group_keys)
    if isinstance(sel, S.IDSelectorAnd):
        return rec(sel.lhs) & rec(sel.rhs)
    if isinstance(sel, S.IDSelectorOr):
        return rec(sel.lhs) | rec(sel.rhs)
    if isinstance(sel, S.IDSelectorXOr):
        return rec(sel.lhs) ^ rec(sel.rhs)
    if isinstance(sel, S.IDSelectorNot):
        return ~rec(sel.sel)
    if isinstance(sel, S.IDSelectorAll):
        return np.ones(n, dtype=bool)
    if isinstance(sel, S.IDSelectorGroups):
        return groups_mask(gid, group_keys, sel.keys)
    if isinstance(sel, S.IDSelectorBitmap):
        return idbits_mask(rid, sel.bits)
    if isinstance(sel, S.IDSelectorRange):
        return (rid >= sel.imin) & (rid < sel.imax)
    if isinstance(sel, S.IDSelectorBatch):                                     # IDSelectorArray too
        return np.isin(rid, sel.ids)
    raise TypeError(type(sel).__name__)


def words(m):
    """uint32[ceil(N / 32)]: bit (p & 31) of word p >> 5 = m[p]; the bits past N are zero"""
    m = np.asarray(m, dtype=bool)
    padded = np.zeros((m.size + 31) // 32 * 32, dtype=bool)
    padded[:m.size] = m
    return np.packbits(padded.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)


def unwords(w, n):
    """the inverse of words: [n] bool (the tail bits are dropped)"""
    return np.unpackbits(np.asarray(w, dtype="<u4").view(np.uint8), bitorder="little")[:n].astype(bool)


def combine(a, b, n, op):
    """wise_sel_combine on uint32 words of n positions: 0 and, 1 or, 2 xor, 3 and-not, 4 not a; the tail of the result is zero"""
    a = np.asarray(a, dtype=np.uint32)
    b = None if b is None else np.asarray(b, dtype=np.uint32)
    out = (a & b, a | b, a ^ b, a & ~b, ~a)[op] if b is not None else ~a
    out = out.astype(np.uint32)
    if n & 31 and out.size:
        out[-1] &= np.uint32((1 << (n & 31)) - 1)
    return out

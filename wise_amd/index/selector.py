"""Search restricted to a set of ids: faiss's IDSelector classes and SearchParameters objects for the HBM-resident indexes.

    D, I = index.search(q, k, params=SearchParameters(sel=IDSelectorBatch(ids)))
    D, I = ivf.search(q, k, params=SearchParametersIVF(sel=IDSelectorNot(IDSelectorRange(0, 1000)), nprobe=64))

  IDSelectorBatch(ids)         the rows whose external id occurs in `ids` (duplicates allowed; ids no row carries select nothing)
  IDSelectorRange(imin, imax)  the rows with imin <= id < imax
  IDSelectorNot(sel)           the complement within the index, of any selector
  IDSelectorAll()              every row
  IDSelectorArray(ids)         IDSelectorBatch under faiss's other name
  IDSelectorBitmap(bits)       the ids whose bit is set in a uint8 array: bit (i & 7) of bits[i >> 3]
  IDSelectorGroups(keys)       the rows whose GROUP key (set_groups: a video's media id) occurs in `keys`; not in faiss
  IDSelectorAnd(lhs, rhs), IDSelectorOr, IDSelectorXOr      trees of the above

    index.search(q, k, params=SearchParameters(sel=IDSelectorAnd(IDSelectorGroups(media_ids), IDSelectorNot(IDSelectorBatch(seen)))))
    index.remove_ids(IDSelectorGroups([media_id]))            # "delete a video"

Resolution is a recursion over the tree (csrc/sel_tree.hip).  A leaf is one launch — two for a group selector, whose keys are first
marked group by group and then looked up row by row through the group tables, so that "inside these 5,000 videos" ships 5,000 keys
and not the millions of vector ids they stand for —, a Not over a leaf folds into the leaf's `invert`, and a node of two children
is one word-by-word pass over their bitmaps.  Every node keeps its own result per index, so a subtree shared by two filters is
resolved once.  Nothing on the way uses an atomic: a tree resolves to the same bits on every run.

A selector says which EXTERNAL ids may be returned; an index turns it into a bitmap over its own row POSITIONS (rows of
FlatIPIndex._X, rows in list order of a ListStore) — uint32[ceil(N / 32)] on the device, bit (p & 31) of word p >> 5 — that its
scan kernels test before a row may compete (csrc/ivf_select.hip: wise_sel_bitmap; the flat index goes on to the ascending list
of set positions, wise_sel_positions).  Resolution runs on the GPU — the batch ids are sorted and de-duplicated by torch.sort on
the device, every row's id is then looked up by its own lane — and its result is kept on the selector per index: the key is the
index object and its row count once pending rows are merged, so adding rows resolves again.
"""
from __future__ import annotations

import weakref
from typing import Optional

import numpy as np
import torch

from .. import _lib

MODE_BATCH, MODE_RANGE = 0, 1        # wise_sel_bitmap's `mode`


class ResolvedSelector:
    """A selector resolved against one index: `bitmap` (device uint32 words, viewed as int32 [ceil(n / 32)]) over the n row
    positions of that index; `positions()` the ascending list of set positions (device int64) built on first use."""

    def __init__(self, bitmap: torch.Tensor, n: int):
        self.bitmap, self.n = bitmap, int(n)
        self._positions: Optional[torch.Tensor] = None

    def positions(self) -> torch.Tensor:
        if self._positions is None:
            lib = _lib.lib()
            dev = self.bitmap.device
            pos = torch.empty(self.n, dtype=torch.int64, device=dev)
            count = torch.zeros(1, dtype=torch.int64, device=dev)
            ws = torch.empty(max(lib.wise_sel_positions_workspace_bytes(self.n), 1), dtype=torch.uint8, device=dev)
            _lib.check(lib.wise_sel_positions(self.bitmap.data_ptr(), self.n, pos.data_ptr(), self.n, count.data_ptr(), ws.data_ptr(),
                                              ws.numel(), _lib.stream_ptr()), "wise_sel_positions")
            # the one host round trip of a resolution (the scan's grid depends on the count); a cached selector never repeats it
            self._positions = pos[:int(count.item())].clone()
        return self._positions


def _leaf_bitmap(ids, id_base: int, n: int, spec, device) -> torch.Tensor:
    """One wise_sel_bitmap launch: the bitmap of a `_spec` over the rows (ids, id_base, n)."""
    mode, sorted_ids, imin, imax, invert = spec
    bitmap = torch.empty((n + 31) // 32, dtype=torch.int32, device=device)
    _lib.check(_lib.lib().wise_sel_bitmap(_lib.ptr(ids), int(id_base), n, mode, _lib.ptr(sorted_ids),
                                          0 if sorted_ids is None else sorted_ids.numel(), imin, imax, int(invert), bitmap.data_ptr(),
                                          _lib.stream_ptr()), "wise_sel_bitmap")
    return bitmap


def _groups_bitmap(tables: dict, n: int, sel_keys: torch.Tensor, invert: bool, device) -> torch.Tensor:
    """wise_sel_bitmap_groups: the rows whose group key occurs in sel_keys (sorted, unique, on the device), from an index's group
    tables (group_search.GroupTables); two launches, the mark bits of the groups in a workspace of G / 8 bytes."""
    lib = _lib.lib()
    G = int(tables["keys"].numel())
    bitmap = torch.empty((n + 31) // 32, dtype=torch.int32, device=device)
    ws = torch.empty(max(int(lib.wise_sel_groups_workspace_bytes(G)), 1), dtype=torch.uint8, device=device)
    _lib.check(lib.wise_sel_bitmap_groups(tables["gid"].data_ptr(), n, tables["keys"].data_ptr(), G, sel_keys.data_ptr(), sel_keys.numel(),
                                          int(invert), bitmap.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               "wise_sel_bitmap_groups")
    return bitmap


def _idbits_bitmap(ids, id_base: int, n: int, bits: torch.Tensor, invert: bool, device) -> torch.Tensor:
    """wise_sel_bitmap_idbits: the rows whose external id has its bit set in `bits` (uint8 on the device, faiss's bit order)."""
    bitmap = torch.empty((n + 31) // 32, dtype=torch.int32, device=device)
    _lib.check(_lib.lib().wise_sel_bitmap_idbits(_lib.ptr(ids), int(id_base), n, bits.data_ptr(), bits.numel(), int(invert),
                                                 bitmap.data_ptr(), _lib.stream_ptr()), "wise_sel_bitmap_idbits")
    return bitmap


OP_AND, OP_OR, OP_XOR, OP_ANDNOT, OP_NOT = range(5)   # wise_sel_combine's `op`


def _combine(a: torch.Tensor, b: Optional[torch.Tensor], n: int, op: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """wise_sel_combine over two bitmaps of n positions into `out` (a new one by default; a or b may be given): one launch."""
    if out is None:
        out = torch.empty_like(a)
    _lib.check(_lib.lib().wise_sel_combine(a.data_ptr(), _lib.ptr(b), n, op, out.data_ptr(), _lib.stream_ptr()), "wise_sel_combine")
    return out


class IDSelector:
    """Base of the selectors.  `resolve(index)` is what the index classes call; a class says how its bitmap is made in `_bitmap`."""

    def __init__(self):
        self._resolved = weakref.WeakKeyDictionary()      # index -> ResolvedSelector

    def _spec(self, device):
        """(mode, sorted unique ids on `device` or None, imin, imax, invert) — wise_sel_bitmap's arguments"""
        raise NotImplementedError

    def _uses_groups(self) -> bool:
        """does the tree under this selector hold an IDSelectorGroups (its bitmap then belongs to one state of the group tables)"""
        return False

    def _bitmap(self, index, rows, invert: bool) -> torch.Tensor:
        """A NEW bitmap (int32 words on the device) of this selector, complemented within the index where `invert`, over
        rows = index._selector_rows().  Here: the single wise_sel_bitmap launch of a selector that has a `_spec`."""
        ids, id_base, n = rows
        mode, sorted_ids, imin, imax, inv = self._spec(index.device)
        return _leaf_bitmap(ids, id_base, n, (mode, sorted_ids, imin, imax, bool(inv) != bool(invert)), index.device)

    def resolve(self, index) -> ResolvedSelector:
        """The bitmap of this selector over the rows of `index` (anything with `_selector_rows()`: the merged external ids on the
        device or None, id_base, row count), cached until the index's row count changes or rows are removed — and, for a tree with
        a group selector in it, until the index's `_rows_version()` moves: group tables of another state are never used."""
        uses_groups = self._uses_groups()
        if uses_groups:                                    # refused before anything else is asked of the index or launched
            IDSelectorGroups._tables(index)
        rows = index._selector_rows()
        ids, id_base, n = rows
        hit = self._resolved.get(index)
        gen = getattr(index, "_mutations", 0)              # remove_ids moves rows under an unchanged array: resolve again
        version = index._rows_version() if uses_groups else None
        if hit is not None and hit.n == n and hit.ids_ptr == _lib.ptr(ids) and hit.gen == gen and hit.version == version:
            return hit
        res = ResolvedSelector(self._bitmap(index, rows, False), n)
        res.ids_ptr, res.gen, res.version = _lib.ptr(ids), gen, version
        self._resolved[index] = res
        return res


def _integers(name: str, values) -> np.ndarray:
    """[n] int64 of an array-like (or tensor) of integers; ValueError for any other dtype"""
    a = np.asarray(values.cpu() if torch.is_tensor(values) else values)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name} must be integers, got {a.dtype}")
    return np.ascontiguousarray(a, dtype=np.int64).reshape(-1)


class IDSelectorBatch(IDSelector):
    def __init__(self, ids):
        super().__init__()
        self.ids = _integers(f"{type(self).__name__}: ids", ids)
        self._sorted = {}                                  # device -> sorted, de-duplicated ids

    def _spec(self, device):
        key = str(device)
        if key not in self._sorted:
            t = torch.from_numpy(self.ids).to(device)
            self._sorted[key] = torch.unique_consecutive(torch.sort(t).values).contiguous()
        return MODE_BATCH, self._sorted[key], 0, 0, False


class IDSelectorArray(IDSelectorBatch):
    """faiss's IDSelectorArray: the same rows as IDSelectorBatch(ids)"""


class IDSelectorRange(IDSelector):
    def __init__(self, imin: int, imax: int):
        super().__init__()
        for v in (imin, imax):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"IDSelectorRange: bounds must be integers, got {type(v).__name__}")
        self.imin, self.imax = int(imin), int(imax)

    def _spec(self, device):
        return MODE_RANGE, None, self.imin, self.imax, False


class IDSelectorAll(IDSelector):
    """faiss's IDSelectorAll: every row (the complement of an empty id list: one wise_sel_bitmap launch, whatever the ids)"""

    def _spec(self, device):
        return MODE_BATCH, None, 0, 0, True


class IDSelectorNot(IDSelector):
    """The complement within the index of any selector.  Over a leaf it folds into that leaf's `invert` (no launch of its own);
    over a compound selector it is one wise_sel_combine pass."""

    def __init__(self, sel: IDSelector):
        super().__init__()
        if not isinstance(sel, IDSelector):
            raise ValueError(f"IDSelectorNot: expected an IDSelector, got {type(sel).__name__}")
        self.sel = sel
        self._groups_below = sel._uses_groups()           # once: a selector's children do not change

    def _spec(self, device):
        mode, sorted_ids, imin, imax, invert = self.sel._spec(device)
        return mode, sorted_ids, imin, imax, not invert

    def _uses_groups(self) -> bool:
        return self._groups_below

    def _bitmap(self, index, rows, invert: bool) -> torch.Tensor:
        return self.sel._bitmap(index, rows, not invert)


class IDSelectorBitmap(IDSelector):
    """faiss's IDSelectorBitmap: id i is selected iff i >= 0, i >> 3 < len(bits) and bit (i & 7) of bits[i >> 3] is set."""

    def __init__(self, bits):
        super().__init__()
        a = np.asarray(bits.cpu() if torch.is_tensor(bits) else bits)
        if a.dtype != np.uint8:
            raise ValueError(f"IDSelectorBitmap: bits must be a uint8 array, got {a.dtype}")
        self.bits = np.ascontiguousarray(a).reshape(-1)
        self._on = {}                                      # device -> the bits there

    def _bitmap(self, index, rows, invert: bool) -> torch.Tensor:
        ids, id_base, n = rows
        key = str(index.device)
        if key not in self._on:
            self._on[key] = torch.from_numpy(self.bits).to(index.device)
        return _idbits_bitmap(ids, id_base, n, self._on[key], invert, index.device)


class IDSelectorGroups(IDSelector):
    """The rows whose GROUP key (set_groups: the media id of a video, a shot, a file) occurs in `keys` — duplicates allowed, keys
    no group carries select nothing.  Resolved on the device against the index's group tables (csrc/sel_tree.hip): the keys travel,
    not the rows' ids.  RuntimeError on an index without tables for its present rows (as search_grouped), NotImplementedError on the
    types that take no groups (the product-quantized types, the Sharded* wrappers, a slice of a sharded index)."""

    def __init__(self, keys):
        super().__init__()
        self.keys = _integers("IDSelectorGroups: keys", keys)
        self._sorted = {}                                  # device -> sorted, de-duplicated keys

    def _uses_groups(self) -> bool:
        return True

    @staticmethod
    def _tables(index) -> dict:
        """the group tables of the index's present rows: the type's refusal of set_groups, or RuntimeError where it holds none"""
        need = getattr(index, "_need_groups", None)
        if need is None:                                   # a Sharded* wrapper
            from .group_search import NO_SHARDED
            raise NotImplementedError(NO_SHARDED)
        return need()

    def _bitmap(self, index, rows, invert: bool) -> torch.Tensor:
        tables = self._tables(index)
        n = rows[2]
        if int(tables["n"]) != n:
            raise RuntimeError(f"IDSelectorGroups: the group tables cover {int(tables['n'])} rows, the index holds {n}")
        key = str(index.device)
        if key not in self._sorted:                        # sorted on the host: what travels is every key once
            self._sorted[key] = torch.from_numpy(np.unique(self.keys)).to(index.device)
        return _groups_bitmap(tables, n, self._sorted[key], invert, index.device)


class _IDSelectorPair(IDSelector):
    """A node of two selectors: each child is resolved (and cached) on its own, then one wise_sel_combine pass joins the two
    bitmaps into a new one; a complement asked of the node is one more pass over that."""
    OP = None

    def __init__(self, lhs: IDSelector, rhs: IDSelector):
        super().__init__()
        for s in (lhs, rhs):
            if not isinstance(s, IDSelector):
                raise ValueError(f"{type(self).__name__}: expected two IDSelectors, got {type(s).__name__}")
        self.lhs, self.rhs = lhs, rhs
        self._groups_below = lhs._uses_groups() or rhs._uses_groups()          # once: a selector's children do not change

    def _uses_groups(self) -> bool:
        return self._groups_below

    def _bitmap(self, index, rows, invert: bool) -> torch.Tensor:
        n = rows[2]
        a = self.lhs.resolve(index).bitmap
        if self.OP == OP_AND and isinstance(self.rhs, IDSelectorNot):          # a AND NOT b: b as it is, the complement in the pass
            out = _combine(a, self.rhs.sel.resolve(index).bitmap, n, OP_ANDNOT)
        else:
            out = _combine(a, self.rhs.resolve(index).bitmap, n, self.OP)
        return _combine(out, None, n, OP_NOT, out=out) if invert else out


class IDSelectorAnd(_IDSelectorPair):
    """faiss's IDSelectorAnd: the rows both selectors select"""
    OP = OP_AND


class IDSelectorOr(_IDSelectorPair):
    """faiss's IDSelectorOr: the rows either selector selects"""
    OP = OP_OR


class IDSelectorXOr(_IDSelectorPair):
    """faiss's IDSelectorXOr: the rows exactly one of the two selects"""
    OP = OP_XOR


class SearchParameters:
    """faiss.SearchParameters: `sel`, an IDSelector (or one already resolved against the index searched), or None."""

    def __init__(self, sel=None):
        if sel is not None and not isinstance(sel, (IDSelector, ResolvedSelector)):
            raise ValueError(f"SearchParameters: sel must be an IDSelector, got {type(sel).__name__}")
        self.sel = sel


class SearchParametersIVF(SearchParameters):
    """faiss.SearchParametersIVF: `nprobe` replaces the index's nprobe for the one call it is passed to."""

    def __init__(self, sel=None, nprobe: Optional[int] = None):
        super().__init__(sel)
        if nprobe is not None and (isinstance(nprobe, bool) or not isinstance(nprobe, (int, np.integer)) or nprobe < 1):
            raise ValueError(f"SearchParametersIVF: nprobe={nprobe!r} must be a positive integer")
        self.nprobe = None if nprobe is None else int(nprobe)


def unpack_params(params, ivf: bool):
    """(sel, nprobe) of a search call's `params`; ValueError for anything that is not a parameter object of the index family."""
    if params is None:
        return None, None
    if not isinstance(params, SearchParameters):
        raise ValueError(f"search: params must be SearchParameters{'IVF' if ivf else ''}, got {type(params).__name__}")
    nprobe = getattr(params, "nprobe", None)
    if nprobe is not None and not ivf:
        raise ValueError("search: nprobe is a parameter of the inverted-file indexes")
    return params.sel, nprobe


def resolve_for(index, sel) -> Optional[ResolvedSelector]:
    """What a search_device does with its `sel`: None stays None, a selector is resolved against the (finalized) index, and a
    ResolvedSelector is checked against the index's row count — one resolved against other rows is a ValueError."""
    if sel is None:
        return None
    if isinstance(sel, IDSelector):
        return sel.resolve(index)
    if not isinstance(sel, ResolvedSelector):
        raise ValueError(f"search: sel must be an IDSelector, got {type(sel).__name__}")
    n = index._selector_rows()[2]
    if sel.n != n:
        raise ValueError(f"search: the selector was resolved against {sel.n} rows, the index holds {n}")
    return sel


def as_selector(within):
    """FeatureSearchIndex's `within`: a selector as it is, an array-like of vector ids as an IDSelectorBatch."""
    return within if isinstance(within, (IDSelector, ResolvedSelector)) else IDSelectorBatch(within)


def within_selector(within=None, within_groups=None):
    """FeatureSearchIndex's `within` and `within_groups` as one selector: None for neither, `as_selector(within)`,
    IDSelectorGroups(within_groups) — an array-like of group keys —, or the IDSelectorAnd of the two (a `within` already resolved
    against an index cannot be joined: ValueError)."""
    if within_groups is None:
        return None if within is None else as_selector(within)
    groups = IDSelectorGroups(within_groups)
    return groups if within is None else IDSelectorAnd(as_selector(within), groups)

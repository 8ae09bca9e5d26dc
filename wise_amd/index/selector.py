"""Search restricted to a set of ids: faiss's IDSelector classes and SearchParameters objects for the HBM-resident indexes.

    D, I = index.search(q, k, params=SearchParameters(sel=IDSelectorBatch(ids)))
    D, I = ivf.search(q, k, params=SearchParametersIVF(sel=IDSelectorNot(IDSelectorRange(0, 1000)), nprobe=64))

  IDSelectorBatch(ids)         the rows whose external id occurs in `ids` (duplicates allowed; ids no row carries select nothing)
  IDSelectorRange(imin, imax)  the rows with imin <= id < imax
  IDSelectorNot(sel)           the complement within the index

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


class IDSelector:
    """Base of the three selectors.  `resolve(index)` is what the index classes call."""

    def __init__(self):
        self._resolved = weakref.WeakKeyDictionary()      # index -> ResolvedSelector

    def _spec(self, device):
        """(mode, sorted unique ids on `device` or None, imin, imax, invert) — wise_sel_bitmap's arguments"""
        raise NotImplementedError

    def resolve(self, index) -> ResolvedSelector:
        """The bitmap of this selector over the rows of `index` (anything with `_selector_rows()`: the merged external ids on the
        device or None, id_base, row count), cached until the index's row count changes or rows are removed."""
        ids, id_base, n = index._selector_rows()
        hit = self._resolved.get(index)
        gen = getattr(index, "_mutations", 0)              # remove_ids moves rows under an unchanged array: resolve again
        if hit is not None and hit.n == n and hit.ids_ptr == _lib.ptr(ids) and hit.gen == gen:
            return hit
        lib = _lib.lib()
        device = index.device
        mode, sorted_ids, imin, imax, invert = self._spec(device)
        bitmap = torch.empty((n + 31) // 32, dtype=torch.int32, device=device)
        _lib.check(lib.wise_sel_bitmap(_lib.ptr(ids), int(id_base), n, mode, _lib.ptr(sorted_ids),
                                       0 if sorted_ids is None else sorted_ids.numel(), imin, imax, int(invert), bitmap.data_ptr(),
                                       _lib.stream_ptr()), "wise_sel_bitmap")
        res = ResolvedSelector(bitmap, n)
        res.ids_ptr, res.gen = _lib.ptr(ids), gen
        self._resolved[index] = res
        return res


class IDSelectorBatch(IDSelector):
    def __init__(self, ids):
        super().__init__()
        a = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"IDSelectorBatch: ids must be integers, got {a.dtype}")
        self.ids = np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
        self._sorted = {}                                  # device -> sorted, de-duplicated ids

    def _spec(self, device):
        key = str(device)
        if key not in self._sorted:
            t = torch.from_numpy(self.ids).to(device)
            self._sorted[key] = torch.unique_consecutive(torch.sort(t).values).contiguous()
        return MODE_BATCH, self._sorted[key], 0, 0, False


class IDSelectorRange(IDSelector):
    def __init__(self, imin: int, imax: int):
        super().__init__()
        for v in (imin, imax):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"IDSelectorRange: bounds must be integers, got {type(v).__name__}")
        self.imin, self.imax = int(imin), int(imax)

    def _spec(self, device):
        return MODE_RANGE, None, self.imin, self.imax, False


class IDSelectorNot(IDSelector):
    def __init__(self, sel: IDSelector):
        super().__init__()
        if not isinstance(sel, IDSelector):
            raise ValueError(f"IDSelectorNot: expected an IDSelector, got {type(sel).__name__}")
        self.sel = sel

    def _spec(self, device):
        mode, sorted_ids, imin, imax, invert = self.sel._spec(device)
        return mode, sorted_ids, imin, imax, not invert


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

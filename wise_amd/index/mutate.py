"""remove_ids and update_index: the parts every index type shares.

  RowCompaction   one removal: the keep bitmap over row positions, its plan (csrc/compact.hip: the kept-row count in front of
                  every 2048-row segment) and the scratch buffer; `rows(t)` compacts one per-row array in place, `rank(pos)`
                  maps positions (list_off) to what they are after the removal.  Every array of an index goes through the SAME
                  plan, so payload, ids, compact rows and scales stay row-aligned.
  remove_bitmap   the bitmap of the rows that STAY, from anything `as_selector` accepts
  plan_update     the id bookkeeping of FeatureSearchIndex.update_index; numpy only

Extra device memory of a removal: the scratch (SCRATCH_BYTES unless the caller says otherwise, never more than the largest
array), two bitmaps of N / 8 bytes and the plan of N / 256 bytes.  It does not grow with the payload.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from .. import _lib
from .selector import as_selector, resolve_for

SCRATCH_BYTES = 64 << 20         # the default workspace of remove_ids


class RowCompaction:
    def __init__(self, keep: torch.Tensor, n: int, scratch_bytes: int):
        """keep: int32 words over n row positions (bit set = the row stays; the bits past n are ignored).  Plans on the device
        and reads the kept count back: the one host round trip of a removal."""
        lib = _lib.lib()
        self.keep, self.n, self.device = keep, int(n), keep.device
        self.scratch_bytes = int(scratch_bytes)
        if self.scratch_bytes < 1:
            raise ValueError("remove_ids: scratch_bytes must be positive")
        self.plan = torch.empty(max(int(lib.wise_compact_plan_entries(self.n)), 1), dtype=torch.int64, device=self.device)
        count = torch.empty(1, dtype=torch.int64, device=self.device)
        _lib.check(lib.wise_compact_plan(_lib.ptr(keep), self.n, self.plan.data_ptr(), count.data_ptr(), _lib.stream_ptr()),
                   "wise_compact_plan")
        self.kept = int(count.item())
        self._scratch: Optional[torch.Tensor] = None

    def _scratch_for(self, nbytes: int) -> torch.Tensor:
        want = max(min(self.scratch_bytes, nbytes), 1)
        if self._scratch is None or self._scratch.numel() < want:
            self._scratch = None                         # release before the larger one is taken
            self._scratch = torch.empty(want, dtype=torch.uint8, device=self.device)
        return self._scratch

    def rows(self, t: torch.Tensor) -> torch.Tensor:
        """Compact t [n, ...] (contiguous, first dimension = row) in place; returns the view of its first `kept` rows."""
        if t.shape[0] != self.n or not t.is_contiguous():
            raise ValueError(f"remove_ids: expected a contiguous array of {self.n} rows, got {tuple(t.shape)}")
        if self.n and self.kept != self.n:
            width = t.numel() // self.n * t.element_size()
            sc = self._scratch_for(t.numel() * t.element_size())
            _lib.check(_lib.lib().wise_compact_rows(t.data_ptr(), self.n, width, self.keep.data_ptr(), self.plan.data_ptr(),
                                                    sc.data_ptr(), min(sc.numel(), self.scratch_bytes), _lib.stream_ptr()),
                       "wise_compact_rows")
        return t[:self.kept]

    def rank(self, pos: torch.Tensor) -> torch.Tensor:
        """[m] int64 positions in [0, n] -> the number of kept rows before each."""
        out = torch.empty_like(pos)
        _lib.check(_lib.lib().wise_compact_rank(_lib.ptr(self.keep), self.n, self.plan.data_ptr(), pos.data_ptr(), pos.numel(),
                                                out.data_ptr(), _lib.stream_ptr()), "wise_compact_rank")
        return out


def remove_bitmap(index, sel) -> Tuple[torch.Tensor, int]:
    """(keep bitmap, row count): `sel` resolved against the merged rows of `index` by the search path's own resolution
    (wise_sel_bitmap), then inverted: the selected rows go.  The tail bits past the row count come out set; the compaction
    kernels ignore them."""
    res = resolve_for(index, as_selector(sel))
    return torch.bitwise_not(res.bitmap), res.n


def start(index, sel, scratch_bytes: Optional[int]) -> Optional[RowCompaction]:
    """The compaction of remove_ids(sel) on `index`, or None when no row goes."""
    keep, n = remove_bitmap(index, sel)
    if n == 0:
        return None
    c = RowCompaction(keep, n, type(index).REMOVE_SCRATCH_BYTES if scratch_bytes is None else scratch_bytes)
    return None if c.kept == n else c


def plan_update(index_ids, store_ids) -> Tuple[np.ndarray, np.ndarray]:
    """(remove_ids, add_mask) that bring an index holding `index_ids` in line with a store holding `store_ids`:
    remove_ids — the ids the index holds and the store does not, ascending; add_mask — bool over store_ids, True where the
    index lacks the id, so that store_rows[add_mask] are the rows to add IN STORE ORDER.  Ids are unique in a feature store;
    a store that repeats one is refused (ValueError), as is an index that does."""
    index_ids = np.ascontiguousarray(index_ids, dtype=np.int64).reshape(-1)
    store_ids = np.ascontiguousarray(store_ids, dtype=np.int64).reshape(-1)
    if np.unique(store_ids).size != store_ids.size:
        raise ValueError("update_index: the feature store holds the same id more than once")
    held = np.unique(index_ids)
    if held.size != index_ids.size:
        raise ValueError("update_index: the index holds the same id more than once")
    remove = np.setdiff1d(held, store_ids, assume_unique=True)
    add_mask = ~np.isin(store_ids, held, assume_unique=True)
    return remove, add_mask

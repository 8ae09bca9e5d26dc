"""What the exhaustive indexes (flat_ip.py, flat_sq.py, flat_l2.py, flat_pq.py) are made of: one row store and the faiss-shaped surface around it.

  RowStore        ONE [N, d] payload tensor of one dtype (fp32 rows, binary16 rows) and its ids: the tensors reserved up front and
                  their fill mark, the chunks added since the last merge, rows adopted as they are, the implicit ids
                  (id_base + row) of adopted rows, and the compaction of a removal.  Pure torch: it works on the host too.
  FlatIndexBase   everything that does not depend on the payload: ntotal, reserve, adopt, remove_ids, the argument handling of
                  add_with_ids, the numpy search / range_search, range_search_device, reconstruct_batch and the exact scan
                  (`_exact_scan`: all rows, or the rows pos[]) over the entry points a subclass names, rows_host, the grow-only
                  workspaces, and the fp32 staging of rows on their way to an encoder (`_staged`).
  FlatCodecIndex  the search of the types of csrc/flat_codec_scan.h (IndexFlatL2, IndexSQfp16, IndexSQfp16L2, IndexSQ8bit), ONE
                  ROUTE: `_finalize`, the queries, then
                    a selector                    -> the exact scan over its positions (`_TOPK[2]`)
                    BATCH_MIN_ROWS rows and BATCH_MIN_QUERIES queries or more, a shape the batched search serves
                    (`_BATCHED[0]` != 0) and `_batch_operands()` not None
                                                  -> the batched search (`_BATCHED[1]`), counted in `_counters`
                    everything else               -> the exact scan over all rows (`_TOPK[1]`), up to 4 queries a pass
                  Every call is rows, `_payload_args()`, [the operands,] N, d, ... in the order of include/wise_hip.h.
                  THE HOOK `_batch_operands()` returns the device tensors the batched entry point takes between the payload and
                  N — built on first use, dropped by the class's `_rows_changed` — or None where they cannot be built.

A subclass keeps the constructor's shape check (`check_codec_shape` under its own name), how rows enter their slot (`_fill`: a
copy, or an encoder over `_staged`), its entry-point names and BATCH_MIN_* values, and whatever it derives from the rows — which
it drops in `_rows_changed`.  FlatIPIndex (shadow routing) and FlatPQIPIndex (tables, query chunks) keep a search_device of their own.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from .. import _lib
from . import group_search as _group
from . import mutate as _mutate
from . import range_search as _range
from .selector import resolve_for, unpack_params


def check_codec_shape(name: str, d: int) -> None:
    """The row widths csrc/flat_codec_scan.h serves; name: the faiss name the message opens with"""
    if d < 16 or d % 16 != 0 or d > 1024:
        raise ValueError(f"{name}: d={d} must be a multiple of 16 in [16, 1024]")


class RowStore:
    def __init__(self, d: int, dtype: torch.dtype, device="cuda", what: Optional[str] = None):
        """what: how adopt's ValueError describes the rows it takes"""
        self.d, self.dtype, self.device = int(d), dtype, torch.device(device)
        self.what = what or f"rows must be contiguous {dtype} [N,{self.d}] on the store's device"
        self.rows: Optional[torch.Tensor] = None     # [n,d] of the merged rows; None before the first merge of an empty store
        self.ids: Optional[torch.Tensor] = None      # [n] int64, None => id_base + row (adopt only)
        self.id_base = 0
        self.n = 0                                   # merged rows and chunks
        self.chunks: List[torch.Tensor] = []
        self.id_chunks: List[torch.Tensor] = []
        self.reserved: Optional[torch.Tensor] = None      # reserve(): the tensors slot() hands out slice by slice
        self.reserved_ids: Optional[torch.Tensor] = None
        self.fill = 0
        self.version = 0                             # counts what changed the rows (slot, adopt, compact): group tables belong to one value

    @property
    def has_ids(self) -> bool:
        """explicit ids are held (8 bytes a row): always, except over rows adopted without any"""
        return self.ids is not None or bool(self.id_chunks)

    def reserve(self, n: int) -> None:
        """Room for n rows up front: slot() then hands out slices of ONE [n,d] tensor instead of queueing chunks that the merge
        would have to duplicate (an index larger than ~40 % of HBM could not be loaded through chunks; load_index knows the row
        count from the file header)."""
        if self.n or self.chunks:
            raise ValueError("reserve: the index already holds rows")
        self.reserved = torch.empty(int(n), self.d, dtype=self.dtype, device=self.device)
        self.reserved_ids = torch.empty(int(n), dtype=torch.int64, device=self.device)
        self.fill = 0

    def slot(self, n: int, ids, what: str = "add_with_ids") -> torch.Tensor:
        """The [n,d] destination of n new rows, which the caller fills: their slice of the reserved tensor where they fit, else a
        fresh chunk (and the reservation is given up: chunks from here on).  ids [n] int64 go in with them."""
        ids = ids if torch.is_tensor(ids) else torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int64))
        if ids.shape != (n,):
            raise ValueError(f"{what}: ids must have one entry per row")
        self.version += 1
        if self.reserved is not None and self.fill + n <= self.reserved.shape[0]:
            a, b = self.fill, self.fill + n
            self.reserved_ids[a:b].copy_(ids)
            self.rows, self.ids = self.reserved[:b], self.reserved_ids[:b]
            self.fill = self.n = b
            return self.reserved[a:b]
        self.reserved = self.reserved_ids = None
        dst = torch.empty(n, self.d, dtype=self.dtype, device=self.device)
        self.chunks.append(dst)
        self.id_chunks.append(ids.to(self.device, torch.int64))
        self.n += n
        return dst

    def adopt(self, rows: torch.Tensor, ids: Optional[torch.Tensor] = None, id_base: int = 0) -> None:
        """Take ownership of rows already resident on the device (no copy).  ids None => id = id_base + row.  Whatever the store
        held — chunks, a reservation — is gone."""
        if (rows.dtype != self.dtype or rows.dim() != 2 or rows.shape[1] != self.d or not rows.is_contiguous() or
                rows.device.type != self.device.type):
            raise ValueError(f"adopt: {self.what}")
        if ids is not None and (ids.dtype != torch.int64 or ids.shape != (rows.shape[0],)):
            raise ValueError("adopt: ids must be int64 [N]")
        self.chunks, self.id_chunks = [], []
        self.reserved = self.reserved_ids = None
        self.rows, self.ids, self.id_base, self.n = rows, ids, int(id_base), rows.shape[0]
        self.version += 1

    def finalize(self) -> None:
        """Merge the chunks behind the rows held so far (implicit ids become explicit once rows with ids follow them); an empty
        store gets empty tensors."""
        if self.chunks:
            held = self.rows is not None
            self.ids = torch.cat(([self.explicit_ids()] if held else []) + self.id_chunks, dim=0).contiguous()
            self.rows = torch.cat(([self.rows] if held else []) + self.chunks, dim=0).contiguous()
            self.chunks, self.id_chunks = [], []
            self.reserved = self.reserved_ids = None
        if self.rows is None:
            self.rows = torch.empty(0, self.d, dtype=self.dtype, device=self.device)
            self.ids = torch.empty(0, dtype=torch.int64, device=self.device)

    def explicit_ids(self) -> torch.Tensor:
        """[rows] int64 ids of the merged rows, the implicit ones written out"""
        if self.ids is not None:
            return self.ids
        return torch.arange(self.rows.shape[0], device=self.device, dtype=torch.int64) + self.id_base

    def compact(self, c: "_mutate.RowCompaction") -> None:
        """One removal over the merged rows and their (explicit) ids, in place: reserved tensors keep their capacity and are filled
        from the new end."""
        self.rows, self.ids = c.rows(self.rows), c.rows(self.ids)
        self.n = c.kept
        self.version += 1
        if self.reserved is not None:
            self.fill = c.kept


class FlatIndexBase(_group.GroupTables):
    REMOVE_SCRATCH_BYTES = _mutate.SCRATCH_BYTES
    metric = "ip"        # "l2" (flat_l2.py): D holds squared distances, ascending; a range hit is dist < thresh
    # entry points of the subclass's payload: (workspace bytes, count pass, fill pass) of range_search, reconstruct_batch's, and
    # (workspace bytes, all rows, the rows pos[]) of the exact scan
    _RANGE: Tuple[str, str, str]
    _RECONSTRUCT: str
    _TOPK: Tuple[str, str, str]
    _GROUP_SCORES: str   # stage 1 of search_grouped (group_search.py)

    def _payload_args(self) -> tuple:
        """What the range and reconstruct entry points of the subclass take right behind the rows: nothing, or the device address
        of what the payload was trained with (IndexSQ8bit's ranges)."""
        return ()

    def __init__(self, d: int, device, dtype: torch.dtype, what: str):
        self.d = int(d)
        self.device = torch.device(device)
        self._store = RowStore(self.d, dtype, self.device, what)
        self._ws: Optional[torch.Tensor] = None
        self.is_trained = True

    # -- the store, under the names the search paths use ---------------------------------------------
    @property
    def ntotal(self) -> int:
        return self._store.n

    _n = ntotal

    @property
    def _ids(self) -> Optional[torch.Tensor]:
        """[N] int64 on device, None => id_base + row"""
        return self._store.ids

    @property
    def id_base(self) -> int:
        return self._store.id_base

    # -- construction ---------------------------------------------------------------------------
    def reserve(self, n: int) -> None:
        """Room for n rows in HBM up front (RowStore.reserve): later adds fill their slice of ONE [n,d] tensor."""
        self._store.reserve(n)

    def _slot(self, n: int, ids, what: str) -> torch.Tensor:
        dst = self._store.slot(n, ids, what)
        self._rows_changed()
        return dst

    def add_with_ids(self, x, ids) -> None:
        """x [n,d] float32, ids [n] int64 (feature_search_index.py:81)."""
        if not torch.is_tensor(x):
            x = np.ascontiguousarray(x, dtype=np.float32)
            if not x.flags.writeable:   # e.g. a read-only memory map of an index file: torch wants a writable buffer
                x = x.copy()
            x = torch.from_numpy(x)
        if x.dim() != 2 or x.shape[1] != self.d:
            raise ValueError(f"add_with_ids: expected [n,{self.d}], got {tuple(x.shape)}")
        self._fill(self._slot(x.shape[0], ids, "add_with_ids"), x)

    def _staged(self, x: torch.Tensor):
        """x [n,d] (host or device) as float32 device chunks of at most ENCODE_BYTES (the subclass's): (start, chunk) pairs.  A
        chunk that is on the device, contiguous and float32 already is a view of x; any other is copied — and converted — through
        ONE staging buffer, so that no fp32 form of the whole input exists in HBM."""
        rows = max(1, self.ENCODE_BYTES // (4 * self.d))
        stage = None
        for s in range(0, x.shape[0], rows):
            part = x[s:s + rows]
            if part.device.type != self.device.type or not part.is_contiguous() or part.dtype != torch.float32:
                if stage is None:
                    stage = torch.empty(min(rows, x.shape[0]), self.d, dtype=torch.float32, device=self.device)
                stage[:part.shape[0]].copy_(part)
                part = stage[:part.shape[0]]
            yield s, part

    def adopt(self, rows: torch.Tensor, ids: Optional[torch.Tensor] = None, id_base: int = 0):
        """Take ownership of rows already resident in HBM (no copy, no conversion). ids None => id = id_base + row."""
        self._store.adopt(rows, ids, id_base)
        self._rows_changed()
        return self

    def _finalize(self) -> None:
        self._store.finalize()

    def remove_ids(self, sel, scratch_bytes: Optional[int] = None) -> int:
        """faiss's Index::remove_ids: drop the rows `sel` selects (an IDSelector, or an array of ids); returns how many went.
        The payload and the ids are compacted in place, in order (csrc/compact.hip: mutate.start), through a scratch of
        `scratch_bytes` (default REMOVE_SCRATCH_BYTES), so the index is byte for byte the one that received only the kept rows; a
        reserved tensor keeps its capacity and later adds fill it from the new end.  What the subclass derived from the rows is
        dropped and rebuilt by the next search that wants it; its counters go on counting."""
        self._finalize()
        if self._store.n:                              # implicit ids stop being id_base + row once a row goes
            self._store.ids = self._store.explicit_ids()
        c = _mutate.start(self, sel, scratch_bytes)
        if c is None:
            return 0
        self._store.compact(c)
        self._compact_extra(c)
        self._rows_changed()
        self._mutations = getattr(self, "_mutations", 0) + 1
        return c.n - c.kept

    def _compact_extra(self, c: "_mutate.RowCompaction") -> None:
        """remove_ids: further per-row arrays of the subclass go through the same plan (flat_pq.py: the compact rows and scales)"""

    def rows_host(self):
        """(payload [N,d], ids [N] int64) on the host: what the index file holds."""
        self._finalize()
        return self._store.rows.cpu().numpy(), self._store.explicit_ids().cpu().numpy()

    # -- search ---------------------------------------------------------------------------------
    def _selector_rows(self):
        """(external ids on the device or None, id_base, row count) of the merged rows: what a selector is resolved against."""
        self._finalize()
        return self._store.ids, self._store.id_base, self._store.n

    def _queries(self, q: torch.Tensor, what: str) -> torch.Tensor:
        if q.dim() != 2 or q.shape[1] != self.d:
            raise ValueError(f"{what}: expected [nq,{self.d}], got {tuple(q.shape)}")
        return q.to(self.device, torch.float32).contiguous()

    def _grown(self, name: str, need: int) -> torch.Tensor:
        """The byte workspace kept under the attribute `name`, at least `need` bytes: it only ever grows."""
        ws = getattr(self, name)
        if ws is None or ws.numel() < need:
            ws = None
            setattr(self, name, None)                  # release before the larger one is taken
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            setattr(self, name, ws)
        return ws

    def _exact_scan(self, lib, q: torch.Tensor, k: int, D: torch.Tensor, I: torch.Tensor, pos: Optional[torch.Tensor] = None) -> None:
        """The exact scan of the queries q [nq >= 1, d] into D / I [nq,k]: over every row (`_TOPK[1]`), or over the rows at the
        ascending positions pos (`_TOPK[2]`: a resolved selector)."""
        bytes_name, all_name, pos_name = self._TOPK
        X, n, nq = self._store.rows, self._store.n, q.shape[0]
        need = getattr(lib, bytes_name)(n if pos is None else pos.numel(), self.d, nq, k)
        if need == 0:
            raise ValueError(f"search: unsupported shape N={n} d={self.d} nq={nq} k={k}")
        ws = self._grown("_ws", need)
        name = all_name if pos is None else pos_name
        over = () if pos is None else (pos.data_ptr(), pos.numel())
        _lib.check(getattr(lib, name)(X.data_ptr(), *self._payload_args(), n, self.d, *over, q.data_ptr(), nq, k, _lib.ptr(self._store.ids),
                                      self._store.id_base, D.data_ptr(), I.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), name)

    def search(self, x, k: int, params=None):
        """faiss signature: x np.ndarray [nq,d] float32 -> (D, I) numpy (feature_search_index.py:113).
        params: SearchParameters(sel=...) restricts the search to the selected ids (selector.py)."""
        sel, _ = unpack_params(params, ivf=False)
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2:
            raise ValueError("search: x must be 2-D")
        q = torch.from_numpy(x).to(self.device)
        D, I = self.search_device(q, int(k)) if sel is None else self.search_device(q, int(k), sel=sel)
        return D.cpu().numpy(), I.cpu().numpy()

    # -- range search ---------------------------------------------------------------------------
    def range_search_device(self, q: torch.Tensor, thresh: float, sel=None, chunk: Optional[int] = None):
        """q [nq,d] fp32 on device -> (lims [nq+1] int64, D fp32, I int64) on the device: every row with score > thresh, each
        query's segment by descending score, ties by ascending row (range_search.py).  The score is the exact scan's over the
        payload, never a shadow copy's.  sel: only the selected rows can be hits (their bitmap is tested in the count pass).
        chunk: queries per workspace chunk (default: what range_search.WORKSPACE_BYTES allows)."""
        lib = _lib.lib()
        self._finalize()
        radius = _range.check_threshold(thresh)
        res = resolve_for(self, sel)
        keep = None if res is None else res.bitmap
        q = self._queries(q, "range_search")
        X, n, d, st = self._store.rows, self._store.n, self.d, _lib.stream_ptr()
        bytes_name, count_name, fill_name = self._RANGE
        bytes_fn, count_fn, fill_fn = getattr(lib, bytes_name), getattr(lib, count_name), getattr(lib, fill_name)
        extra = self._payload_args()

        def stage(qs):
            def count(counts, ws):
                _lib.check(count_fn(X.data_ptr(), *extra, n, d, qs.data_ptr(), qs.shape[0], radius, _lib.ptr(keep), counts.data_ptr(),
                                    ws.data_ptr(), ws.numel(), st), count_name)

            def fill(lims, D, P, ws):
                _lib.check(fill_fn(X.data_ptr(), *extra, n, d, qs.data_ptr(), qs.shape[0], radius, 0, 0, lims.data_ptr(), D.data_ptr(),
                                   P.data_ptr(), ws.data_ptr(), ws.numel(), st), fill_name)
            return count, fill

        return _range.run(q, lambda m: bytes_fn(n, d, m), stage, lambda need: self._grown("_ws", need), self._store.ids,
                          self._store.id_base, chunk, ascending=self.metric == "l2")

    def range_search(self, x, thresh: float, params=None):
        """faiss signature: x np.ndarray [nq,d] float32 -> (lims, D, I) numpy.  params: SearchParameters(sel=...)."""
        sel, _ = unpack_params(params, ivf=False)
        lims, D, I = self.range_search_device(_range.to_numpy(x).to(self.device), thresh, sel=sel)
        return lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()

    # -- grouped search (set_groups, clear_groups, ngroups, the numpy search_grouped: group_search.GroupTables) ----------------
    def _rows_version(self) -> int:
        return self._store.version

    def _group_operands(self, lib, qs: torch.Tensor) -> tuple:
        """What the subclass's *_group_scores entry point takes between d and nq for the queries qs: the queries themselves, or
        what the payload makes of them (IndexSQ8bit: W and q0)."""
        return (qs,)

    def search_grouped_device(self, q: torch.Tensor, k: int, sel=None, chunk: Optional[int] = None):
        """q [nq,d] fp32 on device -> (D [nq,k] fp32, I [nq,k] int64, G [nq,k] int64) on the device, no host sync: the k best
        groups of rows, each with its best row (group_search.py).  The score is the exact scan's over the payload, never a shadow
        copy's.  sel: only the selected rows are candidates (their bitmap is tested in the score pass).  chunk: queries per
        workspace chunk (default: what range_search.WORKSPACE_BYTES allows).  RuntimeError before set_groups."""
        tables = self._need_groups()
        lib = _lib.lib()
        self._finalize()
        res = resolve_for(self, sel)
        keep = None if res is None else res.bitmap
        q = self._queries(q, "search_grouped")
        X, n, d, st, name = self._store.rows, self._store.n, self.d, _lib.stream_ptr(), self._GROUP_SCORES
        fn = getattr(lib, name)

        def scores(qs, ord_ptr):
            operands = self._group_operands(lib, qs)
            _lib.check(fn(_lib.ptr(X), n, d, *(t.data_ptr() for t in operands), qs.shape[0], _lib.ptr(keep), ord_ptr, st), name)

        return _group.run(q, k, tables, scores, lambda need: self._grown("_ws", need), self._store.ids, self._store.id_base,
                          self.metric, chunk)

    def reconstruct_batch(self, ids) -> np.ndarray:
        """the stored rows under the given external ids as float32 (api/routes.py:1078); NaN rows for ids the index does not
        hold."""
        lib = _lib.lib()
        self._finalize()
        qi = torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int64)).to(self.device)
        out = torch.empty(qi.numel(), self.d, dtype=torch.float32, device=self.device)
        rc = getattr(lib, self._RECONSTRUCT)(self._store.rows.data_ptr(), *self._payload_args(), self._store.n, self.d, _lib.ptr(self._store.ids),
                                             self._store.id_base, qi.data_ptr(), qi.numel(), out.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, self._RECONSTRUCT)
        return out.cpu().numpy()


class FlatCodecIndex(FlatIndexBase):
    """The search route of the types of csrc/flat_codec_scan.h (module docstring).  A subclass sets BATCH_MIN_ROWS and
    BATCH_MIN_QUERIES where it records their measurement."""
    BATCH_MIN_ROWS: int
    BATCH_MIN_QUERIES: int
    _BATCHED: Tuple[str, str]        # entry points of the batched search: (workspace bytes, the search)

    def __init__(self, d: int, device, dtype: torch.dtype, what: str):
        super().__init__(d, device, dtype, what)
        self._counters: Optional[torch.Tensor] = None  # device [2] int32: queries answered from the lists / by the exact scan
        self._bws: Optional[torch.Tensor] = None

    def _batch_operands(self) -> Optional[tuple]:
        """THE HOOK (module docstring): the tensors of the batched call between the payload and N, or None."""
        raise NotImplementedError

    def search_device(self, q: torch.Tensor, k: int, sel=None):
        """q [nq,d] fp32 on device -> (D [nq,k] fp32 — squared distances, ascending, under metric "l2" —, I [nq,k] int64) on device,
        no host sync.  BATCH_MIN_QUERIES or more queries over BATCH_MIN_ROWS rows or more go through the matrix-core passes where
        they serve the shape (the same bits); everything else through the exact scan, up to 4 queries a pass.
        sel: an IDSelector (selector.py) — only the rows it selects compete, by the scan over their positions."""
        lib = _lib.lib()
        self._finalize()
        q = self._queries(q, "search")
        nq, k = q.shape[0], int(k)
        D = torch.empty(nq, k, dtype=torch.float32, device=self.device)
        I = torch.empty(nq, k, dtype=torch.int64, device=self.device)
        if nq == 0:
            return D, I
        pos = None if sel is None else resolve_for(self, sel).positions()
        batch = pos is None and self._n >= self.BATCH_MIN_ROWS and nq >= self.BATCH_MIN_QUERIES
        if not (batch and self._batched_scan(lib, q, k, D, I)):
            self._exact_scan(lib, q, k, D, I, pos)
        return D, I

    def _batched_scan(self, lib, q: torch.Tensor, k: int, D: torch.Tensor, I: torch.Tensor) -> bool:
        """The batched search of the queries q into D / I; False where it does not serve the shape or its operands cannot be built."""
        bytes_name, name = self._BATCHED
        n, nq = self._store.n, q.shape[0]
        need = getattr(lib, bytes_name)(n, self.d, nq, k)
        operands = self._batch_operands() if need else None
        if operands is None:
            return False
        bws = self._grown("_bws", need)
        if self._counters is None:
            self._counters = torch.zeros(2, dtype=torch.int32, device=self.device)
        _lib.check(getattr(lib, name)(self._store.rows.data_ptr(), *self._payload_args(), *(t.data_ptr() for t in operands), n, self.d,
                                      q.data_ptr(), nq, k, _lib.ptr(self._store.ids), self._store.id_base, D.data_ptr(), I.data_ptr(),
                                      self._counters.data_ptr(), bws.data_ptr(), bws.numel(), _lib.stream_ptr()), name)
        return True

    def batched_counts(self):
        """(queries answered from the candidate lists, queries handed to the exact scan) over the batched searches of THIS index so
        far.  Synchronises (a diagnostic, not part of the search path)."""
        if self._counters is None:
            return 0, 0
        c = self._counters.cpu()
        return int(c[0]), int(c[1])

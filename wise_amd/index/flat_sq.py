"""faiss-shaped exhaustive inner-product index whose rows live in HBM as IEEE binary16: IndexSQfp16.

Stands where `faiss.IndexIDMap(faiss.IndexScalarQuantizer(d, QT_fp16, METRIC_INNER_PRODUCT))` would stand beside the reference's
`IndexFlatIP` (src/index/feature_search_index.py:47-52): no training, no nprobe, every row scored — at 2 d bytes a row and nothing
else.  The surface is FlatIPIndex's (flat_ip.py); what differs is the payload: ONE [N, d] array of halves serves the single-query
scan (wise_ipsq16_topk) and, as matrix-core operands as loaded, the batched passes (wise_ipsq16_topk_batched).  There are no fp32
rows and no shadow copy, and no entry point of the fp32 flat index is called.

A score is the fixed-order fp32 sum of include/wise_hip.h (the wise_ivfsq16_scan arithmetic without a bias) whichever path
computes it: search, search under a selector, range_search and the batched search return the same bits for the same row.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from .. import _lib
from . import mutate as _mutate
from . import range_search as _range
from .selector import resolve_for, unpack_params


def check_shape(d: int) -> None:
    if d < 16 or d % 16 != 0 or d > 1024:
        raise ValueError(f"IndexSQfp16: d={d} must be a multiple of 16 in [16, 1024]")


def _halves(t: torch.Tensor) -> torch.Tensor:
    """binary16 rows as the float16 tensor the index keeps (int16 bit patterns are viewed, never converted)"""
    if t.dtype == torch.float16:
        return t
    if t.dtype == torch.int16:
        return t.view(torch.float16)
    raise ValueError(f"IndexSQfp16: binary16 rows expected (float16, or int16 bit patterns), got {t.dtype}")


class FlatSQfp16IPIndex:
    # PROVISIONAL: rows from which search_device hands a batch of 3 or more queries to wise_ipsq16_topk_batched.  FlatIPIndex's floor
    # for its shadow passes; provisional because tools/sqfp16_bench.py measured ONE size (10M x 512) and two batch sizes (1 and 256):
    # neither the row count nor the batch size at which the batched search overtakes the exact scan's 4-query passes is measured
    BATCH_MIN_ROWS = 1 << 18
    # queries from which a batch takes the batched search.  Measured at 10M x 512, k = 10 (profiles/sqfp16_bench.json): a batched
    # pass takes 4.8 ms whatever it carries up to 32 queries, the exact scan 2.8 ms per pass of 4 — 3.3 ms at nq = 3, 5.7 ms at 8,
    # 22.6 ms at 32: 8 is the smallest measured batch at which the batched search wins.  One size, so PROVISIONAL like the row floor
    BATCH_MIN_QUERIES = 8
    ENCODE_BYTES = 64 << 20          # fp32 staging of add_with_ids: rows are encoded on the GPU this many bytes at a time

    def __init__(self, d: int, device: str = "cuda"):
        check_shape(d)
        self.d = int(d)
        self.device = torch.device(device)
        self._H: Optional[torch.Tensor] = None       # [N,d] float16 on device: the whole payload
        self._ids: Optional[torch.Tensor] = None     # [N] int64 on device, None => id_base + row (adopt only)
        self.id_base = 0
        self._n = 0
        self._chunks: List[torch.Tensor] = []
        self._id_chunks: List[torch.Tensor] = []
        self._rH = self._rids = None                 # reserve(): the tensors add_with_ids fills slice by slice
        self._rfill = 0
        self._norms: Optional[torch.Tensor] = None   # device [1]: the largest row norm (wise_ipsq16_prepare), built on demand
        self._counters: Optional[torch.Tensor] = None  # device [2] int32: queries answered from the lists / by the exact scan
        self._ws: Optional[torch.Tensor] = None
        self._bws: Optional[torch.Tensor] = None
        self.is_trained = True

    # -- construction ---------------------------------------------------------------------------
    @property
    def ntotal(self) -> int:
        return self._n

    def hbm_bytes(self) -> int:
        """Bytes of HBM the index itself holds: the halves and the ids (workspaces and the encoder's staging are not part of it)."""
        return self._n * (2 * self.d + (8 if self._ids is not None or self._id_chunks else 0))

    def reserve(self, n: int) -> None:
        """Room for n rows up front: add_with_ids then encodes into its slice of ONE [n,d] tensor."""
        if self._n or self._chunks:
            raise ValueError("reserve: the index already holds rows")
        self._rH = torch.empty(int(n), self.d, dtype=torch.float16, device=self.device)
        self._rids = torch.empty(int(n), dtype=torch.int64, device=self.device)
        self._rfill = 0

    def _encode_into(self, x: torch.Tensor, dst: torch.Tensor) -> None:
        """dst [n,d] float16 (device) = binary16(x [n,d] float32, host or device): wise_sq16_encode over chunks staged in HBM, so
        that the fp32 form of the index never exists there."""
        lib = _lib.lib()
        rows = max(1, self.ENCODE_BYTES // (4 * self.d))
        stage = None
        for s in range(0, x.shape[0], rows):
            part = x[s:s + rows]
            if part.device.type != self.device.type or not part.is_contiguous():
                if stage is None:
                    stage = torch.empty(min(rows, x.shape[0]), self.d, dtype=torch.float32, device=self.device)
                stage[:part.shape[0]].copy_(part)
                part = stage[:part.shape[0]]
            _lib.check(lib.wise_sq16_encode(part.data_ptr(), part.shape[0], self.d, dst[s:s + rows].data_ptr(), _lib.stream_ptr()),
                       "wise_sq16_encode")

    def add_with_ids(self, x, ids) -> None:
        """x [n,d] float32, ids [n] int64: the rows are rounded to binary16 on the GPU (numpy's float32 -> float16 cast)."""
        if not torch.is_tensor(x):
            x = np.ascontiguousarray(x, dtype=np.float32)
            if not x.flags.writeable:
                x = x.copy()
            x = torch.from_numpy(x)
        ids = torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int64)) if not torch.is_tensor(ids) else ids
        if x.dim() != 2 or x.shape[1] != self.d:
            raise ValueError(f"add_with_ids: expected [n,{self.d}], got {tuple(x.shape)}")
        if ids.shape != (x.shape[0],):
            raise ValueError("add_with_ids: ids must have one entry per row")
        x = x.to(torch.float32)
        self._norms = None
        n = x.shape[0]
        if self._rH is not None and self._rfill + n <= self._rH.shape[0]:
            a, b = self._rfill, self._rfill + n
            self._encode_into(x, self._rH[a:b])
            self._rids[a:b].copy_(ids)
            self._rfill = b
            self._H, self._ids, self._n = self._rH[:b], self._rids[:b], b
            return
        if self._rH is not None:                     # more rows than reserved: chunks from here on
            self._rH = self._rids = None
        h = torch.empty(n, self.d, dtype=torch.float16, device=self.device)
        self._encode_into(x, h)
        self._chunks.append(h)
        self._id_chunks.append(ids.to(self.device, torch.int64))
        self._n += n

    def add_halves_with_ids(self, h, ids) -> None:
        """h [n,d] binary16 (numpy float16, or a float16 / int16 tensor), ids [n] int64: rows that are already encoded — an index
        file's — go to HBM as they are."""
        h = _halves(h if torch.is_tensor(h) else torch.from_numpy(np.ascontiguousarray(h, dtype=np.float16)))
        ids = torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int64)) if not torch.is_tensor(ids) else ids
        if h.dim() != 2 or h.shape[1] != self.d:
            raise ValueError(f"add_halves_with_ids: expected [n,{self.d}], got {tuple(h.shape)}")
        if ids.shape != (h.shape[0],):
            raise ValueError("add_halves_with_ids: ids must have one entry per row")
        self._norms = None
        n = h.shape[0]
        if self._rH is not None and self._rfill + n <= self._rH.shape[0]:
            a, b = self._rfill, self._rfill + n
            self._rH[a:b].copy_(h)
            self._rids[a:b].copy_(ids)
            self._rfill = b
            self._H, self._ids, self._n = self._rH[:b], self._rids[:b], b
            return
        if self._rH is not None:
            self._rH = self._rids = None
        self._chunks.append(h.to(self.device).contiguous())
        self._id_chunks.append(ids.to(self.device, torch.int64))
        self._n += n

    def adopt(self, H: torch.Tensor, ids: Optional[torch.Tensor] = None, id_base: int = 0) -> "FlatSQfp16IPIndex":
        """Take ownership of binary16 rows already resident in HBM (no copy, no conversion).  ids None => id = id_base + row."""
        H = _halves(H)
        if H.dim() != 2 or H.shape[1] != self.d or not H.is_contiguous() or H.device.type != self.device.type:
            raise ValueError(f"adopt: H must be contiguous binary16 [N,{self.d}] on the index's device")
        if ids is not None and (ids.dtype != torch.int64 or ids.shape != (H.shape[0],)):
            raise ValueError("adopt: ids must be int64 [N]")
        self._chunks, self._id_chunks = [], []
        self._rH = self._rids = None
        self._H, self._ids, self.id_base, self._n = H, ids, int(id_base), H.shape[0]
        self._norms = None
        return self

    def _finalize(self):
        if self._chunks:
            parts = ([self._H] if self._H is not None else []) + self._chunks
            idp = ([self._ids] if self._ids is not None else []) + self._id_chunks
            if self._H is not None and self._ids is None:
                idp = [torch.arange(self._H.shape[0], device=self.device, dtype=torch.int64) + self.id_base] + self._id_chunks
            self._H = torch.cat(parts, dim=0).contiguous()
            self._ids = torch.cat(idp, dim=0).contiguous()
            self._chunks, self._id_chunks = [], []
            self._rH = self._rids = None
        if self._H is None:
            self._H = torch.empty(0, self.d, dtype=torch.float16, device=self.device)
            self._ids = torch.empty(0, dtype=torch.int64, device=self.device)

    REMOVE_SCRATCH_BYTES = _mutate.SCRATCH_BYTES

    def remove_ids(self, sel, scratch_bytes: Optional[int] = None) -> int:
        """faiss's Index::remove_ids: drop the rows `sel` selects (an IDSelector, or an array of ids); returns how many went.
        The halves and the ids are compacted in place, in order (csrc/compact.hip: mutate.start), so the index is byte for byte
        the one that received only the kept rows; a reserved tensor keeps its capacity."""
        self._finalize()
        if self._ids is None and self._n:              # implicit ids stop being id_base + row once a row goes
            self._ids = torch.arange(self._n, device=self.device, dtype=torch.int64) + self.id_base
        c = _mutate.start(self, sel, scratch_bytes)
        if c is None:
            return 0
        self._H, self._ids = c.rows(self._H), c.rows(self._ids)
        self._n = c.kept
        if self._rH is not None:
            self._rfill = c.kept
        self._norms = None
        self._mutations = getattr(self, "_mutations", 0) + 1
        return c.n - c.kept

    # -- search ---------------------------------------------------------------------------------
    def _selector_rows(self):
        """(external ids on the device or None, id_base, row count) of the merged rows: what a selector is resolved against."""
        self._finalize()
        return self._ids, self.id_base, self._n

    def _queries(self, q: torch.Tensor, what: str) -> torch.Tensor:
        if q.dim() != 2 or q.shape[1] != self.d:
            raise ValueError(f"{what}: expected [nq,{self.d}], got {tuple(q.shape)}")
        return q.to(self.device, torch.float32).contiguous()

    def _workspace(self, need: int) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def _ensure_norms(self, lib) -> torch.Tensor:
        if self._norms is None:
            self._norms = torch.zeros(1, dtype=torch.float32, device=self.device)
            _lib.check(lib.wise_ipsq16_prepare(self._H.data_ptr(), self._n, self.d, self._norms.data_ptr(), _lib.stream_ptr()),
                       "wise_ipsq16_prepare")
        return self._norms

    def search_device(self, q: torch.Tensor, k: int, sel=None):
        """q [nq,d] fp32 on device -> (D [nq,k] fp32, I [nq,k] int64) on device, no host sync.
        BATCH_MIN_QUERIES or more queries over BATCH_MIN_ROWS rows or more go through the matrix-core passes where they serve the shape
        (wise_ipsq16_topk_batched: the same bits); everything else through the exact scan, up to 4 queries a pass.
        sel: an IDSelector (selector.py) — only the rows it selects compete, by the scan over their positions."""
        lib = _lib.lib()
        self._finalize()
        q = self._queries(q, "search")
        nq, k = q.shape[0], int(k)
        D = torch.empty(nq, k, dtype=torch.float32, device=self.device)
        I = torch.empty(nq, k, dtype=torch.int64, device=self.device)
        if nq == 0:
            return D, I
        st = _lib.stream_ptr()
        if sel is not None:
            pos = resolve_for(self, sel).positions()
            need = lib.wise_ipsqfp16_topk_workspace_bytes(pos.numel(), self.d, nq, k)
            if need == 0:
                raise ValueError(f"search: unsupported shape N={self._n} d={self.d} nq={nq} k={k}")
            ws = self._workspace(need)
            _lib.check(lib.wise_ipsq16_topk_pos(self._H.data_ptr(), self._n, self.d, pos.data_ptr(), pos.numel(), q.data_ptr(), nq, k,
                                                _lib.ptr(self._ids), self.id_base, D.data_ptr(), I.data_ptr(), ws.data_ptr(),
                                                ws.numel(), st), "wise_ipsq16_topk_pos")
            return D, I
        batch = self._n >= self.BATCH_MIN_ROWS and nq >= self.BATCH_MIN_QUERIES
        need = lib.wise_ipsqfp16_topk_batched_workspace_bytes(self._n, self.d, nq, k) if batch else 0
        if need:
            if self._bws is None or self._bws.numel() < need:
                self._bws = None
                self._bws = torch.empty(need, dtype=torch.uint8, device=self.device)
            if self._counters is None:
                self._counters = torch.zeros(2, dtype=torch.int32, device=self.device)
            norms = self._ensure_norms(lib)
            _lib.check(lib.wise_ipsq16_topk_batched(self._H.data_ptr(), norms.data_ptr(), self._n, self.d, q.data_ptr(), nq, k,
                                                    _lib.ptr(self._ids), self.id_base, D.data_ptr(), I.data_ptr(),
                                                    self._counters.data_ptr(), self._bws.data_ptr(), self._bws.numel(), st),
                       "wise_ipsq16_topk_batched")
            return D, I
        need = lib.wise_ipsqfp16_topk_workspace_bytes(self._n, self.d, nq, k)
        if need == 0:
            raise ValueError(f"search: unsupported shape N={self._n} d={self.d} nq={nq} k={k}")
        ws = self._workspace(need)
        _lib.check(lib.wise_ipsq16_topk(self._H.data_ptr(), self._n, self.d, q.data_ptr(), nq, k, _lib.ptr(self._ids), self.id_base,
                                        D.data_ptr(), I.data_ptr(), ws.data_ptr(), ws.numel(), st), "wise_ipsq16_topk")
        return D, I

    def batched_counts(self):
        """(queries answered from the candidate lists, queries handed to the exact scan) over the batched searches of THIS index so
        far.  Synchronises (a diagnostic, not part of the search path)."""
        if self._counters is None:
            return 0, 0
        c = self._counters.cpu()
        return int(c[0]), int(c[1])

    def search(self, x, k: int, params=None):
        """faiss signature: x np.ndarray [nq,d] float32 -> (D, I) numpy.  params: SearchParameters(sel=...)."""
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
        query's segment by descending score, ties by ascending row (range_search.py).  The score is the exact scan's.  sel: only
        the selected rows can be hits."""
        lib = _lib.lib()
        self._finalize()
        radius = _range.check_threshold(thresh)
        res = resolve_for(self, sel)
        keep = None if res is None else res.bitmap
        q = self._queries(q, "range_search")
        H, n, d, st = self._H, self._n, self.d, _lib.stream_ptr()

        def stage(qs):
            def count(counts, ws):
                _lib.check(lib.wise_ipsq16_range_count(H.data_ptr(), n, d, qs.data_ptr(), qs.shape[0], radius, _lib.ptr(keep),
                                                       counts.data_ptr(), ws.data_ptr(), ws.numel(), st), "wise_ipsq16_range_count")

            def fill(lims, D, P, ws):
                _lib.check(lib.wise_ipsq16_range_fill(H.data_ptr(), n, d, qs.data_ptr(), qs.shape[0], radius, 0, 0, lims.data_ptr(),
                                                      D.data_ptr(), P.data_ptr(), ws.data_ptr(), ws.numel(), st), "wise_ipsq16_range_fill")
            return count, fill

        return _range.run(q, lambda m: lib.wise_ipsqfp16_range_workspace_bytes(n, d, m), stage, self._workspace, self._ids, self.id_base,
                          chunk)

    def range_search(self, x, thresh: float, params=None):
        """faiss signature: x np.ndarray [nq,d] float32 -> (lims, D, I) numpy.  params: SearchParameters(sel=...)."""
        sel, _ = unpack_params(params, ivf=False)
        lims, D, I = self.range_search_device(_range.to_numpy(x).to(self.device), thresh, sel=sel)
        return lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()

    def reconstruct_batch(self, ids) -> np.ndarray:
        """the stored rows under the given external ids, widened to float32 (float32(float16(x)) of what was added); NaN rows for
        ids the index does not hold."""
        lib = _lib.lib()
        self._finalize()
        qi = torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int64)).to(self.device)
        out = torch.empty(qi.numel(), self.d, dtype=torch.float32, device=self.device)
        _lib.check(lib.wise_ipsq16_reconstruct(self._H.data_ptr(), self._n, self.d, _lib.ptr(self._ids), self.id_base, qi.data_ptr(),
                                               qi.numel(), out.data_ptr(), _lib.stream_ptr()), "wise_ipsq16_reconstruct")
        return out.cpu().numpy()

    def rows_host(self):
        """(halves [N,d] float16, ids [N] int64) on the host: what the index file holds."""
        self._finalize()
        ids = self._ids if self._ids is not None else torch.arange(self._n, device=self.device, dtype=torch.int64) + self.id_base
        return self._H.cpu().numpy(), ids.cpu().numpy()

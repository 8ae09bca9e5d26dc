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

from typing import Optional

import numpy as np
import torch

from .. import _lib
from .flat_common import FlatIndexBase
from .selector import resolve_for


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


class FlatSQfp16IPIndex(FlatIndexBase):
    # PROVISIONAL: rows from which search_device hands a batch of 3 or more queries to wise_ipsq16_topk_batched.  FlatIPIndex's floor
    # for its shadow passes; provisional because tools/sqfp16_bench.py measured ONE size (10M x 512) and two batch sizes (1 and 256):
    # neither the row count nor the batch size at which the batched search overtakes the exact scan's 4-query passes is measured
    BATCH_MIN_ROWS = 1 << 18
    # queries from which a batch takes the batched search.  Measured at 10M x 512, k = 10 (profiles/sqfp16_bench.json): a batched
    # pass takes 4.8 ms whatever it carries up to 32 queries, the exact scan 2.8 ms per pass of 4 — 3.3 ms at nq = 3, 5.7 ms at 8,
    # 22.6 ms at 32: 8 is the smallest measured batch at which the batched search wins.  One size, so PROVISIONAL like the row floor
    BATCH_MIN_QUERIES = 8
    ENCODE_BYTES = 64 << 20          # fp32 staging of add_with_ids: rows are encoded on the GPU this many bytes at a time
    _RANGE = ("wise_ipsqfp16_range_workspace_bytes", "wise_ipsq16_range_count", "wise_ipsq16_range_fill")
    _RECONSTRUCT = "wise_ipsq16_reconstruct"         # the halves widened to float32: float32(float16(x)) of what was added

    def __init__(self, d: int, device: str = "cuda"):
        check_shape(d)
        super().__init__(d, device, torch.float16, f"H must be contiguous binary16 [N,{int(d)}] on the index's device")
        self._norms: Optional[torch.Tensor] = None   # device [1]: the largest row norm (wise_ipsq16_prepare), built on demand
        self._counters: Optional[torch.Tensor] = None  # device [2] int32: queries answered from the lists / by the exact scan
        self._bws: Optional[torch.Tensor] = None

    # -- construction ---------------------------------------------------------------------------
    @property
    def _H(self) -> Optional[torch.Tensor]:
        """[N,d] float16 on device: the whole payload"""
        return self._store.rows

    def hbm_bytes(self) -> int:
        """Bytes of HBM the index itself holds: the halves and the ids (workspaces and the encoder's staging are not part of it)."""
        return self._n * (2 * self.d + (8 if self._store.has_ids else 0))

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

    def _fill(self, dst: torch.Tensor, x: torch.Tensor) -> None:
        """add_with_ids: the rows are rounded to binary16 on the GPU (numpy's float32 -> float16 cast)"""
        self._encode_into(x.to(torch.float32), dst)

    def add_halves_with_ids(self, h, ids) -> None:
        """h [n,d] binary16 (numpy float16, or a float16 / int16 tensor), ids [n] int64: rows that are already encoded — an index
        file's — go to HBM as they are."""
        h = _halves(h if torch.is_tensor(h) else torch.from_numpy(np.ascontiguousarray(h, dtype=np.float16)))
        if h.dim() != 2 or h.shape[1] != self.d:
            raise ValueError(f"add_halves_with_ids: expected [n,{self.d}], got {tuple(h.shape)}")
        self._slot(h.shape[0], ids, "add_halves_with_ids").copy_(h)

    def adopt(self, H: torch.Tensor, ids: Optional[torch.Tensor] = None, id_base: int = 0) -> "FlatSQfp16IPIndex":
        """Take ownership of binary16 rows already resident in HBM (no copy, no conversion).  ids None => id = id_base + row."""
        return super().adopt(_halves(H), ids, id_base)

    def _rows_changed(self) -> None:
        self._norms = None

    # -- search ---------------------------------------------------------------------------------
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
            ws = self._grown("_ws", need)
            _lib.check(lib.wise_ipsq16_topk_pos(self._H.data_ptr(), self._n, self.d, pos.data_ptr(), pos.numel(), q.data_ptr(), nq, k,
                                                _lib.ptr(self._ids), self.id_base, D.data_ptr(), I.data_ptr(), ws.data_ptr(),
                                                ws.numel(), st), "wise_ipsq16_topk_pos")
            return D, I
        batch = self._n >= self.BATCH_MIN_ROWS and nq >= self.BATCH_MIN_QUERIES
        need = lib.wise_ipsqfp16_topk_batched_workspace_bytes(self._n, self.d, nq, k) if batch else 0
        if need:
            self._grown("_bws", need)
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
        ws = self._grown("_ws", need)
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

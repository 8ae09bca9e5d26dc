"""faiss-shaped exhaustive indexes over scalar-quantized rows: IndexSQfp16 (binary16 rows, inner product, below), IndexSQfp16L2 (the
same rows under squared L2: FlatSQfp16L2Index behind it) and IndexSQ8bit (one byte per dimension under trained ranges, inner product:
FlatSQ8IPIndex at the end of the file).

IndexSQfp16.

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
from .flat_common import FlatCodecIndex, check_codec_shape


def check_shape(d: int) -> None:
    check_codec_shape("IndexSQfp16", d)


def _halves(t: torch.Tensor) -> torch.Tensor:
    """binary16 rows as the float16 tensor the index keeps (int16 bit patterns are viewed, never converted)"""
    if t.dtype == torch.float16:
        return t
    if t.dtype == torch.int16:
        return t.view(torch.float16)
    raise ValueError(f"IndexSQfp16: binary16 rows expected (float16, or int16 bit patterns), got {t.dtype}")


class FlatSQfp16IPIndex(FlatCodecIndex):
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
    _TOPK = ("wise_ipsqfp16_topk_workspace_bytes", "wise_ipsq16_topk", "wise_ipsq16_topk_pos")
    _BATCHED = ("wise_ipsqfp16_topk_batched_workspace_bytes", "wise_ipsq16_topk_batched")
    _GROUP_SCORES = "wise_ipsq16_group_scores"

    def __init__(self, d: int, device: str = "cuda"):
        check_shape(d)
        super().__init__(d, device, torch.float16, f"H must be contiguous binary16 [N,{int(d)}] on the index's device")
        self._norms: Optional[torch.Tensor] = None   # device [1]: the largest row norm (wise_ipsq16_prepare), built on demand

    # -- construction ---------------------------------------------------------------------------
    @property
    def _H(self) -> Optional[torch.Tensor]:
        """[N,d] float16 on device: the whole payload"""
        return self._store.rows

    def hbm_bytes(self) -> int:
        """Bytes of HBM the index itself holds: the halves and the ids (workspaces and the encoder's staging are not part of it)."""
        return self._n * (2 * self.d + (8 if self._store.has_ids else 0))

    def _fill(self, dst: torch.Tensor, x: torch.Tensor) -> None:
        """add_with_ids: the rows are rounded to binary16 on the GPU (wise_sq16_encode: numpy's float32 -> float16 cast), chunk by
        chunk, so that the fp32 form of the index never exists in HBM"""
        lib = _lib.lib()
        for s, part in self._staged(x):
            _lib.check(lib.wise_sq16_encode(part.data_ptr(), part.shape[0], self.d, dst[s:s + part.shape[0]].data_ptr(),
                                            _lib.stream_ptr()), "wise_sq16_encode")

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
    def _batch_operands(self):
        if self._norms is None:
            self._norms = torch.zeros(1, dtype=torch.float32, device=self.device)
            _lib.check(_lib.lib().wise_ipsq16_prepare(self._H.data_ptr(), self._n, self.d, self._norms.data_ptr(), _lib.stream_ptr()),
                       "wise_ipsq16_prepare")
        return (self._norms,)


# -------------------------------------------------------------------------------------------------------------------------------------
# IndexSQfp16L2
def check_sqfp16_l2_shape(d: int) -> None:
    check_codec_shape("IndexSQfp16L2", d)


class FlatSQfp16L2Index(FlatSQfp16IPIndex):
    """faiss-shaped exhaustive squared-L2 index over binary16 rows: IndexSQfp16L2, the L2 twin of IndexSQfp16.

    Stands where `faiss.IndexIDMap(faiss.IndexScalarQuantizer(d, QT_fp16, METRIC_L2))` would stand.  The payload and everything that
    builds it are FlatSQfp16IPIndex's — ONE [N, d] array of halves, encoded on the GPU chunk by chunk, N (2 d + 8) bytes with the
    ids; what differs is the metric: returned distances are SQUARED L2, ascending, padded with (+3.4028235e38, -1), and a range hit
    is dist < thresh, strictly (FlatL2Index's surface).  A distance is the fixed-order fp32 sum of include/wise_hip.h (THE DISTANCE
    IS A CONTRACT; tests/sqfp16_l2_ref.py restates it) whichever path computes it.  The stored rows serve the exact scan
    (wise_l2sq16_topk) and, as matrix-core operands as loaded, the batched passes (wise_l2sq16_topk_batched): beside the rows
    the batched search keeps one fp32 half-norm per row and the largest row norm (wise_l2sq16_prepare, N 4 bytes), built lazily and
    dropped whenever the rows change.  There is no bf16 copy.
    """
    metric = "l2"
    # PROVISIONAL: the row floor of the siblings, not measured for this type: tools/sqfp16_l2_bench.py measured ONE size (10M x 512)
    BATCH_MIN_ROWS = 1 << 18
    # queries from which a batch takes the batched search.  Measured at 10M x 512, k = 10 (profiles/sqfp16_l2_bench.json): a batched
    # pass takes 4.9 - 5.0 ms whatever it carries up to 32 queries, the exact scan 3.3 ms per pass of 4 - 3.69 ms at nq = 3 (two
    # passes), 3.31 at 4, 6.30 at 8, 24.2 at 32: 8 is the smallest measured batch from which the batched search wins at every larger
    # measured one (5 to 7 were not measured).  The siblings' value, confirmed at that one size
    BATCH_MIN_QUERIES = 8
    _RANGE = ("wise_l2sqfp16_range_workspace_bytes", "wise_l2sq16_range_count", "wise_l2sq16_range_fill")
    _TOPK = ("wise_l2sqfp16_topk_workspace_bytes", "wise_l2sq16_topk", "wise_l2sq16_topk_pos")
    _BATCHED = ("wise_l2sqfp16_topk_batched_workspace_bytes", "wise_l2sq16_topk_batched")
    _GROUP_SCORES = "wise_l2sq16_group_scores"

    def __init__(self, d: int, device: str = "cuda"):
        check_sqfp16_l2_shape(d)
        super().__init__(d, device)
        self._half: Optional[torch.Tensor] = None    # device [N] fp32: |h|^2 / 2 (wise_l2sq16_prepare), built on demand

    def _rows_changed(self) -> None:
        """The half-norms and the largest norm go with the rows they derive from; the next batched search builds them as a fresh
        index over the rows would."""
        self._half = self._norms = None

    def _batch_operands(self):
        if self._norms is None:
            half = torch.empty(self._n, dtype=torch.float32, device=self.device)
            norms = torch.zeros(1, dtype=torch.float32, device=self.device)
            _lib.check(_lib.lib().wise_l2sq16_prepare(self._H.data_ptr(), self._n, self.d, half.data_ptr(), norms.data_ptr(),
                                                      _lib.stream_ptr()), "wise_l2sq16_prepare")
            self._half, self._norms = half, norms
        return self._half, self._norms


# -------------------------------------------------------------------------------------------------------------------------------------
# IndexSQ8bit
def check_sq8_shape(d: int) -> None:
    check_codec_shape("IndexSQ8bit", d)


def _codes(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.uint8:
        raise ValueError(f"IndexSQ8bit: uint8 codes expected, got {t.dtype}")
    return t


class FlatSQ8IPIndex(FlatCodecIndex):
    """faiss-shaped exhaustive inner-product index whose rows live in HBM as ONE BYTE per dimension: IndexSQ8bit.

    Stands where `faiss.IndexIDMap(faiss.IndexScalarQuantizer(d, QT_8bit, METRIC_INNER_PRODUCT))` (RS_minmax, argument 0) would
    stand: codes [N, d] uint8, trained [2 d] fp32 (vmin, then vdiff) and the ids — N (d + 8) + 8 d bytes, no lists, no nprobe.  The
    surface is FlatSQfp16IPIndex's plus the training: `train(x)` or `set_trained(vmin, vdiff)` must come before the first add.  A
    score is q0 + s_0 of include/wise_hip.h (W, q0 of wise_sq_query, the wise_ivfsq_scan arithmetic) whichever path computes it:
    search, search under a selector, range_search and the batched search return the same bits for the same row.
    """
    # PROVISIONAL: rows from which search_device hands a batch to wise_ipsq8_topk_batched.  IndexSQfp16's floor, not measured for this
    # type: tools/sq8_bench.py measured ONE size (10M x 512)
    BATCH_MIN_ROWS = 1 << 18
    # queries from which a batch takes the batched search.  Measured at 10M x 512, k = 10 (profiles/sq8_bench.json): a batched pass
    # takes 3.5 - 3.6 ms whatever it carries up to 32 queries, the exact scan 2.7 ms per pass of 4 - 2.66 ms at nq = 3, 2.69 at 4, 5.35
    # at 8, 21.0 at 32: 8 is the smallest measured batch from which the batched search wins at every larger measured one (the rule
    # IndexFlatL2 recorded).  One size, so PROVISIONAL like the row floor
    BATCH_MIN_QUERIES = 8
    ENCODE_BYTES = 64 << 20          # fp32 staging of train / add_with_ids: rows go through the GPU this many bytes at a time
    _RANGE = ("wise_ipsq8_range_workspace_bytes", "wise_ipsq8_range_count", "wise_ipsq8_range_fill")
    _RECONSTRUCT = "wise_ipsq8_reconstruct"          # faiss's Codec8bit decode: vmin + ((code + 0.5) / 255) vdiff
    _TOPK = ("wise_ipsq8_topk_workspace_bytes", "wise_ipsq8_topk", "wise_ipsq8_topk_pos")
    _BATCHED = ("wise_ipsq8_topk_batched_workspace_bytes", "wise_ipsq8_topk_batched")
    _GROUP_SCORES = "wise_ipsq8_group_scores"

    def __init__(self, d: int, device: str = "cuda"):
        check_sq8_shape(d)
        super().__init__(d, device, torch.uint8, f"codes must be contiguous uint8 [N,{int(d)}] on the index's device")
        self.is_trained = False
        self._trained: Optional[torch.Tensor] = None  # device [2 d] fp32: vmin, then vdiff
        self._norms: Optional[torch.Tensor] = None    # device [1]: the largest code norm (wise_ipsq8_prepare), built on demand

    # -- training -------------------------------------------------------------------------------
    def minmax(self, x, lohi: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The running per-dimension minimum and maximum of rows x [n,d] float32 (n may be 0) folded into lohi (device [2, d]: lo,
        then hi; None: a fresh one holding +3.4028235e38 / -3.4028235e38) by wise_sq_minmax, chunk by chunk.  Exact and order-free:
        the same rows in any chunks, or the MIN / MAX all-reduce of several ranks' results, give the same bits."""
        lib = _lib.lib()
        x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        if x.dim() != 2 or x.shape[1] != self.d:
            raise ValueError(f"minmax: expected [n,{self.d}], got {tuple(x.shape)}")
        fresh = lohi is None
        if fresh:
            lohi = torch.empty(2, self.d, dtype=torch.float32, device=self.device)
        st = _lib.stream_ptr()
        if fresh or x.shape[0] == 0:
            _lib.check(lib.wise_sq_minmax(0, 0, self.d, lohi[0].data_ptr(), lohi[1].data_ptr(), 0 if fresh else 1, st), "wise_sq_minmax")
        for _, part in self._staged(x):
            _lib.check(lib.wise_sq_minmax(part.data_ptr(), part.shape[0], self.d, lohi[0].data_ptr(), lohi[1].data_ptr(), 1, st),
                       "wise_sq_minmax")
        return lohi

    def set_minmax(self, lohi: torch.Tensor) -> None:
        """Train from a minimum and maximum: vmin = lo, vdiff = hi - lo, one fp32 subtraction (wise_sq_train's bits)."""
        lohi = lohi.to(torch.float32)
        if bool((lohi[0] > lohi[1]).any()):            # the minimum and maximum of no rows at all: ranges of zero width at zero
            lohi = torch.zeros_like(lohi)
        self.set_trained(lohi[0], lohi[1] - lohi[0])

    def train(self, x) -> None:
        """faiss's RS_minmax with argument 0 over the rows x [n >= 1, d]: one range per dimension."""
        x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        if x.dim() != 2 or x.shape[1] != self.d or x.shape[0] < 1:
            raise ValueError(f"train: expected [n >= 1,{self.d}], got {tuple(x.shape)}")
        self.set_minmax(self.minmax(x))

    def set_trained(self, vmin, vdiff) -> None:
        """The ranges as they are (an index file's): vmin [d], vdiff [d] float32.  Only an empty index is trained."""
        if self._n:
            raise RuntimeError("IndexSQ8bit: the index holds rows encoded against its ranges; they cannot change")
        as_t = lambda v: (v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))).to(torch.float32).reshape(-1)
        vmin, vdiff = as_t(vmin), as_t(vdiff)
        if vmin.numel() != self.d or vdiff.numel() != self.d:
            raise ValueError(f"set_trained: vmin and vdiff must hold {self.d} values each")
        self._trained = torch.cat([vmin.to(self.device), vdiff.to(self.device)]).contiguous()
        self.is_trained = True

    def trained_host(self):
        """(vmin [d], vdiff [d]) float32 on the host: what the index file holds."""
        self._need_trained("trained_host")
        t = self._trained.cpu().numpy()
        return t[:self.d].copy(), t[self.d:].copy()

    def _need_trained(self, what: str) -> None:
        if not self.is_trained:
            raise RuntimeError(f"IndexSQ8bit: {what} before train() or set_trained()")

    def _payload_args(self) -> tuple:
        return (self._trained.data_ptr(),)

    # -- construction ---------------------------------------------------------------------------
    @property
    def _codes_t(self) -> Optional[torch.Tensor]:
        """[N,d] uint8 on device: the whole payload"""
        return self._store.rows

    def hbm_bytes(self) -> int:
        """Bytes of HBM the index itself holds: the codes, the ids and the ranges."""
        return self._n * (self.d + (8 if self._store.has_ids else 0)) + 8 * self.d

    def add_with_ids(self, x, ids) -> None:
        self._need_trained("add_with_ids")
        super().add_with_ids(x, ids)

    def _fill(self, dst: torch.Tensor, x: torch.Tensor) -> None:
        """add_with_ids: the rows are encoded on the GPU (wise_sq_encode; values outside the trained ranges clamp), chunk by chunk,
        so that no fp32 form of the index exists in HBM"""
        lib = _lib.lib()
        for s, part in self._staged(x):
            _lib.check(lib.wise_sq_encode(part.data_ptr(), self._trained.data_ptr(), part.shape[0], self.d,
                                          dst[s:s + part.shape[0]].data_ptr(), _lib.stream_ptr()), "wise_sq_encode")

    def add_codes_with_ids(self, codes, ids) -> None:
        """codes [n,d] uint8 (numpy or tensor), ids [n] int64: rows that are already encoded — an index file's — go to HBM as they
        are."""
        self._need_trained("add_codes_with_ids")
        c = _codes(codes if torch.is_tensor(codes) else torch.from_numpy(np.array(codes, dtype=np.uint8, order="C")))
        if c.dim() != 2 or c.shape[1] != self.d:
            raise ValueError(f"add_codes_with_ids: expected [n,{self.d}], got {tuple(c.shape)}")
        self._slot(c.shape[0], ids, "add_codes_with_ids").copy_(c)

    def adopt(self, codes: torch.Tensor, ids: Optional[torch.Tensor] = None, id_base: int = 0) -> "FlatSQ8IPIndex":
        """Take ownership of codes already resident in HBM (no copy).  ids None => id = id_base + row."""
        self._need_trained("adopt")
        return super().adopt(_codes(codes), ids, id_base)

    def _rows_changed(self) -> None:
        self._norms = None

    def range_search_device(self, q, thresh, sel=None, chunk=None):
        self._need_trained("range_search")
        return super().range_search_device(q, thresh, sel=sel, chunk=chunk)

    def reconstruct_batch(self, ids) -> np.ndarray:
        self._need_trained("reconstruct_batch")
        return super().reconstruct_batch(ids)

    def _group_operands(self, lib, qs: torch.Tensor) -> tuple:
        """(W, q0) of wise_sq_query for the queries: what wise_ipsq8_topk makes of them in its workspace"""
        self._need_trained("search_grouped")
        W = torch.empty(qs.shape[0], self.d, dtype=torch.float32, device=self.device)
        q0 = torch.empty(qs.shape[0], dtype=torch.float32, device=self.device)
        _lib.check(lib.wise_sq_query(qs.data_ptr(), self._trained.data_ptr(), qs.shape[0], self.d, W.data_ptr(), q0.data_ptr(),
                                     _lib.stream_ptr()), "wise_sq_query")
        return W, q0

    # -- search ---------------------------------------------------------------------------------
    def _batch_operands(self):
        if self._norms is None:
            self._norms = torch.zeros(1, dtype=torch.float32, device=self.device)
            _lib.check(_lib.lib().wise_ipsq8_prepare(self._codes_t.data_ptr(), self._n, self.d, self._norms.data_ptr(), _lib.stream_ptr()),
                       "wise_ipsq8_prepare")
        return (self._norms,)

    def search_device(self, q: torch.Tensor, k: int, sel=None):
        self._need_trained("search")
        return super().search_device(q, k, sel=sel)

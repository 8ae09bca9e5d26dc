"""faiss-shaped exhaustive squared-L2 index whose rows live in HBM as fp32: IndexFlatL2.

Stands where `faiss.IndexIDMap(faiss.IndexFlatL2(d))` would stand beside the reference's `IndexFlatIP`
(src/index/feature_search_index.py:47-52): no training, every row scored, N d 4 bytes like IndexFlatIP.  For embeddings that are
not normalised — where L2 and the inner product rank differently — and for anything that expects faiss's L2 surface: returned
distances are SQUARED L2, ascending, padded with (+3.4028235e38, -1) when fewer than k rows compete, and a range hit is
dist < thresh, strictly.

A distance is the fixed-order fp32 sum of include/wise_hip.h (THE DISTANCE IS A CONTRACT; tests/l2_flat_ref.py restates it)
whichever path computes it: search, search under a selector, range_search and the batched search return the same bits for the
same row.  On the device everything selects on the score -dist, so keys, ties (the lower position wins) and merges are the
inner-product types'.

One query, and any small batch, goes through the exact scan (wise_l2_topk_f32), up to 4 queries a pass, N d 4 bytes a pass: there
is no reduced-precision first stage for a single query.  For batches the class keeps, built lazily and dropped whenever the rows
change, a bf16 copy of the rows (+50 % memory) and one fp32 half-norm |x|^2 / 2 per row (wise_l2_prepare), which the matrix-core
passes of wise_l2_topk_batched read instead of the fp32 rows.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from .flat_common import FlatCodecIndex, check_codec_shape


def check_shape(d: int) -> None:
    check_codec_shape("IndexFlatL2", d)


class FlatL2Index(FlatCodecIndex):
    metric = "l2"
    # PROVISIONAL: rows from which search_device hands a batch to wise_l2_topk_batched (below it the bf16 copy is never built).
    # FlatSQfp16IPIndex's floor; tools/flatl2_bench.py measured ONE size (10M x 512), so the row count at which the batched search
    # overtakes the exact scan's 4-query passes is not measured
    BATCH_MIN_ROWS = 1 << 18
    # queries from which a batch takes the batched search.  Measured at 10M x 512, k = 10 (profiles/flatl2_bench.json): a batched
    # pass takes 5.2 ms whatever it carries up to 32 queries, the exact scan 3.7 ms per pass of 4 — 6.5 ms at nq = 3 (two passes),
    # 3.75 ms at 4, 7.5 ms at 8, 29.6 ms at 32: 8 is the smallest measured batch from which the batched search wins at every larger
    # one (5 to 7 were not measured).  FlatSQfp16IPIndex's value, confirmed at that one size
    BATCH_MIN_QUERIES = 8
    _RANGE = ("wise_l2_range_workspace_bytes", "wise_l2_range_count_f32", "wise_l2_range_fill_f32")
    _RECONSTRUCT = "wise_reconstruct_batch"          # the fp32 rows as they were added
    _TOPK = ("wise_l2_topk_workspace_bytes", "wise_l2_topk_f32", "wise_l2_topk_pos_f32")
    _BATCHED = ("wise_l2_topk_batched_workspace_bytes", "wise_l2_topk_batched")
    _GROUP_SCORES = "wise_l2_group_scores_f32"

    def __init__(self, d: int, device: str = "cuda"):
        check_shape(d)
        super().__init__(d, device, torch.float32, "X must be contiguous float32 [N,d]")
        self._Xb: Optional[torch.Tensor] = None      # [N,d] bf16 bits (int16) on device
        self._half: Optional[torch.Tensor] = None    # [N] fp32: |x|^2 / 2
        self._norms: Optional[torch.Tensor] = None   # device [2]: largest row norm, largest bf16 rounding-residual norm

    @property
    def _X(self):
        """[N,d] fp32 on device: the whole payload"""
        return self._store.rows

    def hbm_bytes(self) -> int:
        """Bytes of HBM the index itself holds: the rows and the ids (workspaces are not part of it)."""
        return self._n * (4 * self.d + (8 if self._store.has_ids else 0))

    def _fill(self, dst: torch.Tensor, x: torch.Tensor) -> None:
        dst.copy_(x)                               # host -> its slice of the reserved tensor (or its chunk), no intermediate

    def _rows_changed(self) -> None:
        """The bf16 copy, the half-norms and the two norms go with the rows they derive from; the next batched search builds them as
        a fresh index over the rows would."""
        self._Xb = self._half = self._norms = None

    def _batch_operands(self):
        """(Xb, half, norms) of wise_l2_topk_batched, built if they are not there; None (and the batched route switched off for
        this index) when HBM has no room for them."""
        if self._Xb is None:
            free, _ = torch.cuda.mem_get_info(self.device)
            if free < self._n * (2 * self.d + 4) + (2 << 30):       # keep 2 GiB for workspaces and the caller
                self.BATCH_MIN_ROWS = 1 << 62
                return None
            Xb = torch.empty(self._n, self.d, dtype=torch.int16, device=self.device)
            half = torch.empty(self._n, dtype=torch.float32, device=self.device)
            norms = torch.zeros(2, dtype=torch.float32, device=self.device)
            _lib.check(_lib.lib().wise_l2_prepare(self._X.data_ptr(), self._n, self.d, Xb.data_ptr(), half.data_ptr(), norms.data_ptr(),
                                                  _lib.stream_ptr()), "wise_l2_prepare")
            self._Xb, self._half, self._norms = Xb, half, norms
        return self._Xb, self._half, self._norms

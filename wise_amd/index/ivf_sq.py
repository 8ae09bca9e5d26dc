"""faiss-shaped IVF index (inner product) whose lists hold one byte per dimension: 8-bit scalar-quantized residuals.

Stands where `faiss.IndexIVFScalarQuantizer(IndexFlatIP(d), d, nlist, faiss.ScalarQuantizer.QT_8bit, METRIC_INNER_PRODUCT)`
stands (by_residual = True, the faiss default; index type 'IndexIVFSQ8').  HBM holds N * (d + 8) bytes of codes and ids, the
centroids [nlist, d] and one range per dimension (vmin, vdiff: 8 d bytes) — no codebooks, no per-query table, no second copy of
the rows.  It is the one-byte-per-dimension point of the family: IndexIVFPQ<m> stops at m = 128 bytes per row because its
per-query table is m KiB of LDS.

  coarse stage        the CoarseQuantizer and ListStore of the other inverted-file types (ivf_common.py); building the lists,
                      the search around the scan and its rank-local form are CodedIVFIndexBase's, shared with ivf_pq.py
  train(x)            coarse k-means, then vmin[i] = min r_i, vdiff[i] = max r_i - vmin[i] over the residuals r = x - c_l of the
                      training rows (wise_sq_train): faiss's RS_minmax with argument 0, an exact reduction
  add_with_ids(x,ids) code_i = clamp(floor((r_i - vmin[i]) * (255 / vdiff[i])), 0, 255) (wise_sq_encode), only the codes are kept.
                      The formula is evaluated in float64, so a value inside the trained range lands in the bin it really
                      falls into and decodes to within half a bin.  faiss computes (int)(255 * ((r - vmin) / vdiff)) in
                      float32: the two differ only in rounding at a bin edge.  THE DECODER AND THE FILE ARE faiss's (Codec8bit, the 'IwSq' record of faiss_io.py)
  search(q, k)        probes from the coarse stage, bias = q . c_l (wise_pq_bias), per query w[i] = q_i vdiff[i] / 255 and
                      q0 = sum_i q_i (vmin[i] + vdiff[i] 0.5 / 255) (wise_sq_query), then wise_ivfsq_scan:
                      score = (bias + q0) + sum_i w[i] * code_i in the order include/wise_hip.h fixes.  One stage: a selector
                      (sel=) restricts the same scan (wise_ivfsq_scan_sel)
  reconstruct_batch   decoded, hence approximate, as in faiss: c_l + vmin + vdiff (code + 0.5) / 255 (wise_sq_decode)
What is exact and tested: given the same centroids, ranges and codes the scan equals a float32 restatement bit for bit
(tests/ivfsq_ref.py), and so do the trainer, the encoder and the decoder.

Across GPUs (sharded.py: ShardedIVFSQIPIndex) an index holds ONE RANK's slice of the list-major arrays: all centroids and the
ranges, list_off clipped to the slice, and `pos_base`, the position of its first row in the whole array.  `search_local_device`
is then the rank's share of a search (wise_ivfsq_scan_local: only the probed lists the rank holds), `encode_rows` hands a rank's
rows back as codes for the collective build, and `reconstruct_batch` decodes the ids the slice holds (NaN for the others).

IVFSQfp16IPIndex (index type 'IndexIVFSQfp16') is the two-bytes-per-dimension point of the same family: faiss's QT_fp16.  A row is
its residual cast to IEEE binary16 (wise_sq16_encode: numpy's float32 -> float16 cast), N * (2 d + 8) bytes in all.  Nothing is
trained beyond the centroids, so there is no `trained` state, no weight row and no q0: the query itself is the weight and a search
has one launch fewer — probes, bias, then wise_ivfsq16_scan with score = bias + sum_i q_i * (float)h_i in the order
include/wise_hip.h fixes (tests/ivfsqfp16_ref.py restates it).  It is IVFSQIPIndex with those differences and nothing else: the
list store, the selector, range_search, remove_ids, the rank-local scan and the sharded wrapper are shared.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import _lib
from .ivf_common import CodedIVFIndexBase, _as_tensor, _rows_f32

MAX_D = 1024


def check_sq_shape(d: int) -> None:
    """The shapes wise_sq_* / wise_ivfsq_scan serve (include/wise_hip.h); ValueError otherwise."""
    if d % 16 or d < 16 or d > MAX_D:
        raise ValueError(f"IVFSQIPIndex: d={d} must be a multiple of 16 in [16, {MAX_D}] (a row is read in 16-byte loads)")


def _gather_codes(codes: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """rows of d bytes or 2 d bytes (whole multiples of 16) moved as rows of floats: the copy does not look at the values"""
    out = torch.empty_like(codes)
    _lib.check(_lib.lib().wise_ivf_gather_rows(codes.data_ptr(), idx.data_ptr(), idx.shape[0], codes.shape[1] * codes.element_size() // 4,
                                               out.data_ptr(), _lib.stream_ptr()), "wise_ivf_gather_rows")
    return out


class IVFSQIPIndex(CodedIVFIndexBase):
    # what IVFSQfp16IPIndex replaces: the payload's dtype and the entry points of the C ABI
    PAYLOAD_DTYPE = torch.uint8
    SCAN, SCAN_SEL, SCAN_LOCAL = "wise_ivfsq_scan", "wise_ivfsq_scan_sel", "wise_ivfsq_scan_local"
    WORKSPACE, WORKSPACE_LOCAL = "wise_ivfsq_scan_workspace_bytes", "wise_ivfsq_scan_local_workspace_bytes"
    RANGE_COUNT, RANGE_FILL = "wise_ivfsq_range_count", "wise_ivfsq_range_fill"
    GROUP_SCORES = "wise_ivfsq_group_scores"

    def __init__(self, d: int, nlist: int, device: str = "cuda"):
        check_sq_shape(int(d))
        super().__init__(d, nlist, device, width=int(d), dtype=self.PAYLOAD_DTYPE, gather=_gather_codes)
        self.trained: Optional[torch.Tensor] = None        # [2 d] fp32: vmin, then vdiff

    @property
    def is_trained(self) -> bool:
        return self._coarse.is_trained and self.trained is not None

    def hbm_bytes(self) -> int:
        """Bytes of HBM the index holds once its lists are merged: codes, ids, offsets, centroids, ranges."""
        self._finalize()
        return self._lists.nbytes() + sum(t.numel() * t.element_size() for t in (self.centroids, self.trained) if t is not None)   # (fp16: no ranges)

    # -- training -------------------------------------------------------------------------------
    def train(self, x) -> None:
        x = _rows_f32(x, self.d, "train")
        self._coarse.train(x)
        x = x.to(self.device, torch.float32).contiguous()
        resid = self._residuals(x, self._coarse.assign_device(x, self.centroids))
        trained = torch.empty(2 * self.d, dtype=torch.float32, device=self.device)
        _lib.check(_lib.lib().wise_sq_train(resid.data_ptr(), resid.shape[0], self.d, trained.data_ptr(), _lib.stream_ptr()),
                   "wise_sq_train")
        self.trained = trained

    def set_trained(self, vmin, vdiff) -> None:
        """Install trained ranges, vmin [d] and vdiff [d] (file load, tests)."""
        vmin, vdiff = _as_tensor(vmin, np.float32), _as_tensor(vdiff, np.float32)
        if tuple(vmin.shape) != (self.d,) or tuple(vdiff.shape) != (self.d,):
            raise ValueError(f"set_trained: expected vmin [{self.d}] and vdiff [{self.d}]")
        self.trained = torch.cat([vmin.to(self.device, torch.float32), vdiff.to(self.device, torch.float32)]).contiguous()

    # -- construction (add_with_ids, encode_rows, adopt_lists: CodedIVFIndexBase) ------------------
    def _encode(self, resid: torch.Tensor) -> torch.Tensor:
        codes = torch.empty(resid.shape[0], self.d, dtype=torch.uint8, device=self.device)
        _lib.check(_lib.lib().wise_sq_encode(resid.data_ptr(), self.trained.data_ptr(), resid.shape[0], self.d, codes.data_ptr(),
                                             _lib.stream_ptr()), "wise_sq_encode")
        return codes

    def _payload(self, xs: torch.Tensor, assign: torch.Tensor) -> torch.Tensor:
        return self._encode(self._residuals(xs, assign))

    # -- search (_scan, search_device, search_local_device: CodedIVFIndexBase) ---------------------
    def _operands(self, lib, st: int, qs: torch.Tensor) -> tuple:
        """What the scan entry points take between ids and nq: (W, q0) of wise_sq_query."""
        W = torch.empty(qs.shape[0], self.d, dtype=torch.float32, device=self.device)
        q0 = torch.empty(qs.shape[0], dtype=torch.float32, device=self.device)
        _lib.check(lib.wise_sq_query(qs.data_ptr(), self.trained.data_ptr(), qs.shape[0], self.d, W.data_ptr(), q0.data_ptr(), st),
                   "wise_sq_query")
        return W, q0

    def _range_workspace_bytes(self, nq: int, nprobe: int) -> int:
        return _lib.lib().wise_ivfsq_range_workspace_bytes(self._lists.n, self.nlist, nq, nprobe)

    def _range_stage(self, qs, probes, nprobe, radius, keep):
        """bias and operands as _scan computes them, then wise_ivfsq_range_count / _fill over the same probes"""
        lib, ls, st, n = _lib.lib(), self._lists, _lib.stream_ptr(), qs.shape[0]
        bias = self._bias(lib, st, qs, probes, nprobe)
        weights = self._operands(lib, st, qs)
        head = (ls.data.data_ptr(), ls.n, self.d, ls.list_off.data_ptr(), self.nlist)

        def mid():       # built inside the closures: they, not this frame, keep the weights, probes and bias alive until fill has run
            return (*(t.data_ptr() for t in weights), n, probes.data_ptr(), bias.data_ptr(), nprobe, radius)

        def count(counts, ws):
            _lib.check(getattr(lib, self.RANGE_COUNT)(*head, *mid(), _lib.ptr(keep), counts.data_ptr(), ws.data_ptr(), ws.numel(), st),
                       self.RANGE_COUNT)

        def fill(lims, D, P, ws):
            _lib.check(getattr(lib, self.RANGE_FILL)(*head, 0, *mid(), lims.data_ptr(), D.data_ptr(), P.data_ptr(), ws.data_ptr(),
                                                     ws.numel(), st), self.RANGE_FILL)
        return count, fill

    def _group_scores(self, lib, st, qs, probes, nprobe, keep, ord_ptr) -> None:
        """bias and operands as _scan computes them, then the GROUP_SCORES call over the same probes"""
        ls = self._lists
        bias = self._bias(lib, st, qs, probes, nprobe)
        weights = self._operands(lib, st, qs)
        _lib.check(getattr(lib, self.GROUP_SCORES)(ls.data.data_ptr(), ls.n, self.d, ls.list_off.data_ptr(), self.nlist,
                                                   *(t.data_ptr() for t in weights), qs.shape[0], probes.data_ptr(), bias.data_ptr(), nprobe,
                                                   _lib.ptr(keep), ord_ptr, st), self.GROUP_SCORES)

    # -- the rest of the surface the REST layer touches -------------------------------------------
    def reconstruct_batch(self, ids) -> np.ndarray:
        """Decoded rows (approximate, as faiss's): centroid of the row's list + the bin centres; NaN for an unknown id."""
        pos = self._positions(ids)
        out = torch.empty(pos.numel(), self.d, dtype=torch.float32, device=self.device)
        self._decode(pos, out)
        return out.cpu().numpy()

    def _decode(self, pos: torch.Tensor, out: torch.Tensor) -> None:
        ls = self._lists
        _lib.check(_lib.lib().wise_sq_decode(ls.data.data_ptr(), ls.n, pos.data_ptr(), pos.numel(), ls.list_off.data_ptr(), self.nlist,
                                             self.centroids.data_ptr(), self.trained.data_ptr(), self.d, out.data_ptr(),
                                             _lib.stream_ptr()), "wise_sq_decode")

    def lists_host(self):
        """(centroids [nlist,d], trained [2d] = vmin then vdiff, codes [N,d] uint8, ids [N], list_off [nlist+1]) as numpy."""
        self._finalize()
        ls = self._lists
        return (self.centroids.cpu().numpy(), self.trained.cpu().numpy(), ls.data.cpu().numpy(), ls.ids.cpu().numpy(),
                ls.list_off.cpu().numpy())

    def state_host(self) -> dict:
        """The index as the dict faiss_io.read_ivf_sq_ip returns and faiss_io.write_index takes."""
        return dict(zip(("centroids", "trained", "codes", "ids", "list_off"), self.lists_host()), nprobe=self.nprobe)


class IVFSQfp16IPIndex(IVFSQIPIndex):
    """Index type 'IndexIVFSQfp16' (module docstring): the rows as binary16 residuals, `halves` [N, d] float16.  No `trained`
    state: is_trained is the coarse quantizer's alone, train() runs the coarse k-means only."""
    PAYLOAD_DTYPE = torch.float16
    SCAN, SCAN_SEL, SCAN_LOCAL = "wise_ivfsq16_scan", "wise_ivfsq16_scan_sel", "wise_ivfsq16_scan_local"
    RANGE_COUNT, RANGE_FILL = "wise_ivfsq16_range_count", "wise_ivfsq16_range_fill"
    GROUP_SCORES = "wise_ivfsq16_group_scores"

    @property
    def is_trained(self) -> bool:
        return self._coarse.is_trained

    def train(self, x) -> None:
        self._coarse.train(_rows_f32(x, self.d, "train"))

    def set_trained(self, vmin, vdiff) -> None:
        raise TypeError("IVFSQfp16IPIndex has no trained ranges")

    def _encode(self, resid: torch.Tensor) -> torch.Tensor:
        halves = torch.empty(resid.shape[0], self.d, dtype=torch.float16, device=self.device)
        _lib.check(_lib.lib().wise_sq16_encode(resid.data_ptr(), resid.shape[0], self.d, halves.data_ptr(), _lib.stream_ptr()),
                   "wise_sq16_encode")
        return halves

    def _operands(self, lib, st: int, qs: torch.Tensor) -> tuple:
        return (qs,)                                     # the query is the weight row; there is no q0

    def _decode(self, pos: torch.Tensor, out: torch.Tensor) -> None:
        ls = self._lists
        _lib.check(_lib.lib().wise_sq16_decode(ls.data.data_ptr(), ls.n, pos.data_ptr(), pos.numel(), ls.list_off.data_ptr(), self.nlist,
                                               self.centroids.data_ptr(), self.d, out.data_ptr(), _lib.stream_ptr()), "wise_sq16_decode")

    def lists_host(self):
        """(centroids [nlist,d], halves [N,d] float16, ids [N], list_off [nlist+1]) as numpy."""
        self._finalize()
        ls = self._lists
        return self.centroids.cpu().numpy(), ls.data.cpu().numpy(), ls.ids.cpu().numpy(), ls.list_off.cpu().numpy()

    def state_host(self) -> dict:
        """The index as the dict faiss_io.read_ivf_sq_ip returns for a QT_fp16 file and faiss_io.write_index takes."""
        return dict(zip(("centroids", "halves", "ids", "list_off"), self.lists_host()), nprobe=self.nprobe)

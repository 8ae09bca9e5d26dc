"""faiss-shaped IVF index (inner product) whose lists hold 8-bit product-quantizer codes instead of fp32 rows.

Stands where `faiss.IndexIVFPQ(IndexFlatIP(d), d, nlist, m, 8, METRIC_INNER_PRODUCT)` stands (by_residual = True, the faiss
default): the index family of the reference's own index study (docs/Search-Index-Evaluation.md:105-123).  HBM holds
N * (m + 8) bytes of codes and ids, the centroids [nlist, d] and the codebooks [m, 256, d / m] — and no fp32 rows.

  coarse stage        the CoarseQuantizer and ListStore IVFFlatIPIndex has (ivf_common.py): the same spherical k-means,
                      `probes_device`, list bookkeeping; building the lists, the search around the scan and its rank-local
                      form are CodedIVFIndexBase's, shared with ivf_sq.py
  train(x)            coarse k-means, then per sub-space Lloyd k-means (L2, plain means, 10 iterations) on the residuals of at
                      most 65,536 training rows drawn by a seeded host permutation whose first 256 rows are the initial
                      codewords; an empty codeword keeps its value; deterministic (wise_pq_encode / wise_pq_update)
  add_with_ids(x,ids) rows are assigned to a list, their residuals encoded (wise_pq_encode), and only the codes are kept
  search(q, k)        probes from the coarse stage, bias = q . c_l (wise_pq_bias), one table per query (wise_pq_lut),
                      wise_ivfpq_scan: score = bias + sum_j lut[j][code_j], added in that order in fp32
  reconstruct_batch   decoded, hence approximate, as in faiss: c_l + concat_j cb[j][code_j]
What is exact and tested: given the same centroids, codebooks and codes the scan equals a float32 restatement bit for bit
(tests/ivfpq_ref.py); the trainer is held to the same restatement's distortion.

IVFPQRefineIPIndex (index types IndexIVFPQ<m>R8 / IndexIVFPQ<m>R16) is the same index with a re-ranking stage, faiss's
IndexRefine: the rows are also kept in list order as compact rows — int8 with a scale per row (d + 4 bytes) or bf16 (2 d bytes),
built per chunk by wise_ip_shadow_i8 / wise_ip_shadow_bf16 — and a search takes the k * k_factor best positions of the PQ scan
and scores them again from those rows (wise_ivf_refine, bit-equal to tests/ivfpq_refine_ref.py).  reconstruct_batch returns the
dequantised stored row.

IVFOPQIPIndex / IVFOPQRefineIPIndex (index types IndexIVFOPQ<m>, IndexIVFOPQ<m>R8 / R16) put a learned orthonormal rotation R
[d, d] in front of the product quantizer — faiss's OPQMatrix, as in 'OPQ64,IVF65536,PQ64'.  With r = x - c_l,
q . x = q . c_l + (R q) . (R r), so only three things change: rows are encoded from R r, the per-query table is built from R q
(both wise_opq_rotate), and the no-store type's reconstruct_batch undoes the rotation (wise_opq_decode: c_l + R^T cw).  The
coarse stage, the bias, both scans and the re-ranking stage read what they read before.  Training alternates codebooks and
rotation on the same training residuals: from R = I, opq_niter = 50 times {rotate; fit the codebooks — the first time exactly
train_codebooks, later opq_niter_pq = 4 Lloyd iterations from where they stand; encode; M = sum_i cw_i x_i^T (wise_opq_corr,
fp64); R = U V^T from M = U S V^T}, then one more rotation and fit.  THE SVD IS numpy.linalg.svd IN FLOAT64 ON THE HOST, once
per outer iteration: d x d work (at most 1024 x 1024), not a hot path, and robust when M is rank-deficient.  It is the one
place in the index code where a LAPACK routine does arithmetic, and it is there by decision.

Across GPUs (sharded.py: ShardedIVFPQIPIndex / ShardedIVFPQRefineIPIndex) an index holds ONE RANK's slice of the list-major
arrays: all centroids and codebooks, list_off clipped to the slice, and `pos_base`, the position of its first row in the whole
array.  `search_local_device` is then the rank's share of a search (wise_ivfpq_scan_local: only the probed lists the rank holds),
and the re-ranking index offers its two phases separately — `candidates_local_device` (positions in the whole array) and
`refine_local_device` (wise_ivf_refine_local: candidates outside the slice are holes).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import _lib
from .ivf_common import CodedIVFIndexBase, _as_tensor, _rows_f32

KSUB = 256
MAX_TRAIN_ROWS = 256 * KSUB      # faiss caps a sub-quantizer's training set at 256 rows per codeword


def check_pq_shape(d: int, m: int, nbits: int = 8) -> None:
    """The shapes wise_pq_* serve (include/wise_hip.h); ValueError otherwise."""
    if nbits != 8:
        raise ValueError(f"IVFPQIPIndex: nbits={nbits}: only 8-bit codes are built")
    if m < 1 or m > 128:
        raise ValueError(f"IVFPQIPIndex: m={m} out of [1, 128] (the per-query table is m KiB of the CU's LDS)")
    if d % m != 0:
        raise ValueError(f"IVFPQIPIndex: d={d} is not a multiple of m={m}")
    dsub = d // m
    if dsub % 2 or dsub < 2 or dsub > 96:
        raise ValueError(f"IVFPQIPIndex: d / m = {dsub} must be even and in [2, 96]")


def _gather_codes(codes: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(codes)
    _lib.check(_lib.lib().wise_pq_gather_codes(codes.data_ptr(), idx.data_ptr(), idx.shape[0], codes.shape[1], out.data_ptr(),
                                               _lib.stream_ptr()), "wise_pq_gather_codes")
    return out


def _gather_wide(rows: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """compact rows (whole multiples of 16 bytes) moved as rows of floats: the copy does not look at the values"""
    out = torch.empty_like(rows)
    _lib.check(_lib.lib().wise_ivf_gather_rows(rows.data_ptr(), idx.data_ptr(), idx.shape[0], rows.shape[1] * rows.element_size() // 4,
                                               out.data_ptr(), _lib.stream_ptr()), "wise_ivf_gather_rows")
    return out


def _gather_scales(scales: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """[n] fp32 moved as rows of 4 bytes"""
    out = torch.empty_like(scales)
    _lib.check(_lib.lib().wise_pq_gather_codes(scales.data_ptr(), idx.data_ptr(), idx.shape[0], 4, out.data_ptr(), _lib.stream_ptr()),
               "wise_pq_gather_codes")
    return out


class PQCodebooks:
    """The codebook trainer the product-quantizer indexes share (IVFPQIPIndex trains on residuals, flat_pq.py's FlatPQIPIndex on
    the rows themselves): what it is given are `resid` [n, d] fp32 rows on the device, in training order.  The index supplies d, m,
    dsub, device, niter and the attribute `codebooks`."""

    def _encode(self, resid: torch.Tensor, codebooks: torch.Tensor) -> torch.Tensor:
        codes = torch.empty(resid.shape[0], self.m, dtype=torch.uint8, device=self.device)
        _lib.check(_lib.lib().wise_pq_encode(resid.data_ptr(), codebooks.data_ptr(), resid.shape[0], self.d, self.m, codes.data_ptr(),
                                             _lib.stream_ptr()), "wise_pq_encode")
        return codes

    def _update(self, resid: torch.Tensor, codes: torch.Tensor, cb_in: torch.Tensor) -> torch.Tensor:
        cb_out = torch.empty_like(cb_in)
        _lib.check(_lib.lib().wise_pq_update(resid.data_ptr(), codes.data_ptr(), resid.shape[0], self.d, self.m, cb_in.data_ptr(),
                                             cb_out.data_ptr(), _lib.stream_ptr()), "wise_pq_update")
        return cb_out

    def initial_codebooks(self, resid: torch.Tensor) -> torch.Tensor:
        """[m, 256, dsub]: codeword c of every sub-space = the sub-vector of residual row c (one Lloyd update in which row c
        alone is assigned to codeword c: the slicing is the library's, not a torch permute)."""
        first = resid[:KSUB].contiguous()
        codes = torch.arange(KSUB, dtype=torch.uint8, device=self.device).unsqueeze(1).expand(KSUB, self.m).contiguous()
        return self._update(first, codes, torch.zeros(self.m, KSUB, self.dsub, dtype=torch.float32, device=self.device))

    def train_codebooks(self, resid: torch.Tensor, codebooks: Optional[torch.Tensor] = None) -> torch.Tensor:
        """niter Lloyd iterations from `codebooks` (default: initial_codebooks(resid))."""
        cb = self.initial_codebooks(resid) if codebooks is None else codebooks
        for _ in range(self.niter):
            cb = self._update(resid, self._encode(resid, cb), cb)
        return cb

    def set_codebooks(self, codebooks) -> None:
        """Install trained codebooks [m, 256, dsub] (file load, tests)."""
        cb = _as_tensor(codebooks, np.float32)
        if tuple(cb.shape) != (self.m, KSUB, self.dsub):
            raise ValueError(f"set_codebooks: expected [{self.m},{KSUB},{self.dsub}]")
        self.codebooks = cb.to(self.device, torch.float32).contiguous()


class IVFPQIPIndex(PQCodebooks, CodedIVFIndexBase):
    SCAN, SCAN_SEL, SCAN_LOCAL = "wise_ivfpq_scan", "wise_ivfpq_scan_sel", "wise_ivfpq_scan_local"
    WORKSPACE, WORKSPACE_LOCAL = "wise_ivfpq_scan_workspace_bytes", "wise_ivfpq_scan_local_workspace_bytes"
    WHO = "IVFPQIPIndex"                                 # the subclasses' "train() before ..." texts carry this name too

    def __init__(self, d: int, nlist: int, m: int, nbits: int = 8, device: str = "cuda", extra_gathers=()):
        check_pq_shape(int(d), int(m), int(nbits))
        super().__init__(d, nlist, device, width=int(m), dtype=torch.uint8, gather=_gather_codes, extra_gathers=extra_gathers)
        self.m, self.nbits = int(m), 8
        self._workspace_extra, self._shape_suffix = (self.m,), f" m={self.m}"
        self.dsub = self.d // self.m
        self.niter = 10           # of the codebook training; the coarse k-means keeps its own
        self.seed = 1234
        self.codebooks: Optional[torch.Tensor] = None      # [m, 256, dsub] fp32

    @property
    def is_trained(self) -> bool:
        return self._coarse.is_trained and self.codebooks is not None

    def hbm_bytes(self) -> int:
        """Bytes of HBM the index holds once its lists are merged: codes, ids, offsets, centroids, codebooks."""
        self._finalize()
        return self._lists.nbytes() + sum(t.numel() * t.element_size() for t in (self.centroids, self.codebooks))

    # -- training (the codebook trainer: PQCodebooks) -----------------------------------------------
    def training_residuals(self, x: torch.Tensor) -> torch.Tensor:
        """The residuals the codebooks are trained on: rows perm[:65536] of x (seeded host permutation), in that order."""
        n = x.shape[0]
        perm = np.random.default_rng(self.seed).permutation(n)[:MAX_TRAIN_ROWS].astype(np.int64)
        xs = self._coarse._gather_rows(x, torch.from_numpy(perm).to(self.device))
        return self._residuals(xs, self._coarse.assign_device(xs, self.centroids))

    def train(self, x) -> None:
        x = _rows_f32(x, self.d, "train")
        if x.shape[0] < KSUB:
            raise ValueError(f"train: {x.shape[0]} training vectors for {KSUB} codewords")
        self._coarse.train(x)
        x = x.to(self.device, torch.float32).contiguous()
        self.codebooks = self.train_codebooks(self.training_residuals(x))

    # -- construction (add_with_ids, encode_rows, adopt_lists: CodedIVFIndexBase) ------------------
    def _payload(self, xs: torch.Tensor, assign: torch.Tensor) -> torch.Tensor:
        return self._encode(self._code_input(xs, assign), self.codebooks)

    def _code_input(self, xs: torch.Tensor, assign: torch.Tensor) -> torch.Tensor:
        """What the codes of a chunk of rows are encoded from: the residuals (IVFOPQIPIndex: the rotated residuals)."""
        return self._residuals(xs, assign)

    def _table_queries(self, qs: torch.Tensor) -> torch.Tensor:
        """What the per-query tables are built from: the queries (IVFOPQIPIndex: the rotated queries)."""
        return qs

    # -- search (_scan, search_device, search_local_device: CodedIVFIndexBase) ---------------------
    def _operands(self, lib, st: int, qs: torch.Tensor) -> tuple:
        """What the scan entry points take between ids and nq: one table per query (wise_pq_lut), [n, m, 256] fp32."""
        lut = torch.empty(qs.shape[0], self.m, KSUB, dtype=torch.float32, device=self.device)
        tq = self._table_queries(qs)
        _lib.check(lib.wise_pq_lut(tq.data_ptr(), self.codebooks.data_ptr(), qs.shape[0], self.d, self.m, lut.data_ptr(), st),
                   "wise_pq_lut")
        return (lut,)

    # -- the rest of the surface the REST layer touches -------------------------------------------
    def reconstruct_batch(self, ids) -> np.ndarray:
        """Decoded rows (approximate, as faiss's): centroid of the row's list + its codewords; NaN for an unknown id."""
        lib = _lib.lib()
        pos = self._positions(ids)
        st, ls = _lib.stream_ptr(), self._lists
        out = torch.empty(pos.numel(), self.d, dtype=torch.float32, device=self.device)
        _lib.check(lib.wise_pq_decode(ls.data.data_ptr(), ls.n, pos.data_ptr(), pos.numel(), ls.list_off.data_ptr(), self.nlist,
                                      self.centroids.data_ptr(), self.codebooks.data_ptr(), self.d, self.m, out.data_ptr(), st),
                   "wise_pq_decode")
        return out.cpu().numpy()

    def lists_host(self):
        """(centroids [nlist,d], codebooks [m,256,dsub], codes [N,m] uint8, ids [N], list_off [nlist+1]) as numpy."""
        self._finalize()
        ls = self._lists
        return (self.centroids.cpu().numpy(), self.codebooks.cpu().numpy(), ls.data.cpu().numpy(), ls.ids.cpu().numpy(),
                ls.list_off.cpu().numpy())

    def state_host(self) -> dict:
        """The index as the dict the faiss_io reader of its file returns and faiss_io.write_index takes: read_ivf_pq_ip's keys;
        the re-ranking classes add their store (rows of kind 16 as uint16 bit patterns), the OPQ classes their rotation."""
        return dict(zip(("centroids", "codebooks", "codes", "ids", "list_off"), self.lists_host()), nprobe=self.nprobe)


REFINE_KINDS = (8, 16)
MAX_CANDIDATES = 2048            # the most positions one scan returns and one wise_ivf_refine call takes
# The smallest k_factor of {1, 2, 5, 10, 20, 50, 100, 200} whose recall@10 is within 0.01 of the largest one's.
# PROVISIONAL: 50 is what the CPU study of tests/golden/ivfpq_refine_quality.json shows (60,000 rows); the sweep of
# tools/ivfpq_refine_bench.py on an MI355X (profiles/ivfpq_refine_bench.json) has not been run yet.
DEFAULT_K_FACTOR = 50


def check_refine_shape(d: int, kind: int) -> None:
    """The stores wise_ivf_refine serves, which are the shapes the two builders take (include/wise_hip.h); ValueError otherwise."""
    if kind not in REFINE_KINDS:
        raise ValueError(f"IVFPQRefineIPIndex: kind={kind}: the stores are 8 (int8 rows + a scale each) and 16 (bf16 rows)")
    step = 16 if kind == 8 else 8
    if d % step or d < step or d > 1024:
        raise ValueError(f"IVFPQRefineIPIndex: d={d} must be a multiple of {step} in [{step}, 1024] for the {kind}-bit store")


class IVFPQRefineIPIndex(IVFPQIPIndex):
    """IVFPQIPIndex + compact rows in list order + a re-ranking stage (module docstring).  `k_factor` as on faiss's IndexRefine:
    a search for k re-ranks the min(k * k_factor, 2048) best positions of the PQ scan."""

    def __init__(self, d: int, nlist: int, m: int, kind: int, k_factor: int = DEFAULT_K_FACTOR, device: str = "cuda"):
        check_refine_shape(int(d), int(kind))
        super().__init__(d, nlist, m, device=device, extra_gathers=(_gather_wide, _gather_scales) if kind == 8 else (_gather_wide,))
        self.kind = int(kind)
        self.k_factor = int(k_factor)

    @property
    def _row_dtype(self) -> torch.dtype:
        return torch.int8 if self.kind == 8 else torch.int16          # int16: bf16 bit patterns

    def _extra_rows(self, xs: torch.Tensor) -> tuple:
        lib, st = _lib.lib(), _lib.stream_ptr()
        rows = torch.empty(xs.shape, dtype=self._row_dtype, device=self.device)
        norms = torch.empty(4, dtype=torch.float32, device=self.device)      # the builders' error norms: scratch, not used here
        if self.kind == 8:
            scales = torch.empty(xs.shape[0], dtype=torch.float32, device=self.device)
            _lib.check(lib.wise_ip_shadow_i8(xs.data_ptr(), xs.shape[0], self.d, rows.data_ptr(), scales.data_ptr(), norms.data_ptr(), st),
                       "wise_ip_shadow_i8")
            return rows, scales
        _lib.check(lib.wise_ip_shadow_bf16(xs.data_ptr(), xs.shape[0], self.d, rows.data_ptr(), norms.data_ptr(), st), "wise_ip_shadow_bf16")
        return (rows,)

    def adopt_lists(self, codes: torch.Tensor, ids: torch.Tensor, list_off: torch.Tensor, rows: torch.Tensor = None,
                    scales: torch.Tensor = None, pos_base: int = 0) -> "IVFPQRefineIPIndex":
        """Take codes and compact rows that are already grouped by list (file load); pos_base as on IVFPQIPIndex."""
        return super().adopt_lists(codes, ids, list_off, pos_base, (rows, scales))

    def _adopted_extra(self, n: int, rows, scales) -> tuple:
        if rows is None or tuple(rows.shape) != (n, self.d) or rows.dtype != self._row_dtype:
            raise ValueError(f"adopt_lists: expected rows [{n},{self.d}] {self._row_dtype}")
        if self.kind == 8 and (scales is None or tuple(scales.shape) != (n,) or scales.dtype != torch.float32):
            raise ValueError(f"adopt_lists: expected scales [{n}] float32")
        return (rows, scales) if self.kind == 8 else (rows,)

    def _store(self):
        """(rows pointer, scales pointer or 0) of the merged lists"""
        ex = self._lists.extra
        return ex[0].data_ptr(), ex[1].data_ptr() if self.kind == 8 else 0

    def candidates(self, k: int) -> int:
        """How many positions of the PQ scan a search for k re-ranks."""
        return max(k, min(k * max(self.k_factor, 1), MAX_CANDIDATES))

    def search_device(self, q: torch.Tensor, k: int, chunk: int = 1024, sel=None):
        """sel: an IDSelector — the candidates are the k * k_factor best SELECTED rows of the PQ scan; the re-ranking is unchanged."""
        lib = _lib.lib()
        q = self._queries(q)
        keep = self._keep(sel)
        if k < 1 or k > MAX_CANDIDATES:
            raise ValueError(f"search: unsupported k={k} (1 <= k <= {MAX_CANDIDATES})")
        nq, kc, ls, st = q.shape[0], self.candidates(k), self._lists, _lib.stream_ptr()
        D = torch.empty(nq, k, dtype=torch.float32, device=self.device)
        I = torch.empty(nq, k, dtype=torch.int64, device=self.device)
        if ls.n == 0:
            return D.fill_(-3.4028234663852886e38), I.fill_(-1)
        rows, scales = self._store()
        for s in range(0, nq, chunk):
            qs = q[s:s + chunk]
            n = qs.shape[0]
            cD = torch.empty(n, kc, dtype=torch.float32, device=self.device)
            cand = torch.empty(n, kc, dtype=torch.int64, device=self.device)
            self._scan(qs, kc, cD, cand, positions=True, keep=keep)
            _lib.check(lib.wise_ivf_refine(rows, self.kind, scales, ls.n, self.d, ls.ids.data_ptr(), qs.data_ptr(), n, cand.data_ptr(),
                                           kc, k, D[s:s + chunk].data_ptr(), I[s:s + chunk].data_ptr(), st), "wise_ivf_refine")
        return D, I

    def search_local_device(self, q, k, probe_count=None, positions=False, chunk: int = 1024):
        raise NotImplementedError("IVFPQRefineIPIndex: a rank's share of a search is two phases, candidates_local_device and "
                                  "refine_local_device, with an exchange between them (ShardedIVFPQRefineIPIndex)")

    def candidates_local_device(self, q: torch.Tensor, kc: int, probe_count: Optional[torch.Tensor] = None, chunk: int = 1024):
        """Phase 1 of a sharded search: this slice's kc best rows of the PQ scan as (scores, positions in the WHOLE array)."""
        if kc < 1 or kc > MAX_CANDIDATES:
            raise ValueError(f"candidates_local_device: unsupported kc={kc} (1 <= kc <= {MAX_CANDIDATES})")
        return self._search(q, kc, chunk, True, True, probe_count)

    def refine_local_device(self, q: torch.Tensor, cand: torch.Tensor, k: int):
        """Phase 2: the candidates cand [nq, kc] (positions in the whole array, the same on every rank) that lie in this slice,
        scored again from its compact rows; the k best with external ids (wise_ivf_refine_local)."""
        q = self._queries(q)
        nq, ls = q.shape[0], self._lists
        if cand.dim() != 2 or cand.shape[0] != nq or cand.dtype != torch.int64 or cand.shape[1] > MAX_CANDIDATES:
            raise ValueError(f"refine_local_device: cand must be int64 [{nq}, kc <= {MAX_CANDIDATES}]")
        if k < 1 or k > MAX_CANDIDATES:
            raise ValueError(f"refine_local_device: unsupported k={k} (1 <= k <= {MAX_CANDIDATES})")
        cand = cand.to(self.device).contiguous()
        D = torch.empty(nq, k, dtype=torch.float32, device=self.device)
        I = torch.empty(nq, k, dtype=torch.int64, device=self.device)
        if ls.n == 0:
            return D.fill_(-3.4028234663852886e38), I.fill_(-1)
        rows, scales = self._store()
        _lib.check(_lib.lib().wise_ivf_refine_local(rows, self.kind, scales, ls.n, self.d, ls.ids.data_ptr(), q.data_ptr(), nq,
                                                    cand.data_ptr(), cand.shape[1], k, self.pos_base, D.data_ptr(), I.data_ptr(),
                                                    _lib.stream_ptr()), "wise_ivf_refine_local")
        return D, I

    def reconstruct_batch(self, ids) -> np.ndarray:
        """The stored rows, dequantised (faiss's IndexRefine reconstructs from its refine index too); NaN for an unknown id."""
        pos = self._positions(ids)
        out = torch.empty(pos.numel(), self.d, dtype=torch.float32, device=self.device)
        if self._lists.n == 0:
            return out.fill_(float("nan")).cpu().numpy()
        rows, scales = self._store()
        _lib.check(_lib.lib().wise_ivf_refine_rows(rows, self.kind, scales, self._lists.n, self.d, pos.data_ptr(), pos.numel(),
                                                   out.data_ptr(), _lib.stream_ptr()), "wise_ivf_refine_rows")
        return out.cpu().numpy()

    def store_host(self):
        """(rows [N,d] int8 or uint16 bf16 bits, scales [N] float32 or None) of the merged lists as numpy."""
        self._finalize()
        ex = self._lists.extra
        if self._lists.n == 0:
            return np.empty((0, self.d), dtype=np.int8 if self.kind == 8 else np.uint16), (np.empty(0, np.float32) if self.kind == 8 else None)
        rows = ex[0].cpu().numpy()
        return (rows, ex[1].cpu().numpy()) if self.kind == 8 else (rows.view(np.uint16), None)

    def state_host(self) -> dict:
        rows, scales = self.store_host()
        return dict(super().state_host(), kind=self.kind, k_factor=self.k_factor, rows=rows, scales=scales)


MAX_OPQ_D = 1024                 # wise_opq_rotate keeps 32 rows of d floats in LDS


def check_opq_shape(d: int, m: int) -> None:
    """The shapes wise_opq_* serve on top of check_pq_shape (include/wise_hip.h); ValueError otherwise."""
    check_pq_shape(d, m)
    if d % 4 or d < 4 or d > MAX_OPQ_D:
        raise ValueError(f"IVFOPQIPIndex: d={d} must be a multiple of 4 in [4, {MAX_OPQ_D}] (the rotation is d x d)")


class _OPQRotation:
    """What turns an IVFPQ index into its OPQ form: the rotation, its trainer, and the two places it enters — the rows are
    encoded from R (x - c_l), the per-query tables are built from R q.  Mixed in front of IVFPQIPIndex / IVFPQRefineIPIndex."""

    def _init_rotation(self) -> None:
        check_opq_shape(self.d, self.m)
        self.opq_niter = 50          # outer iterations (faiss OPQMatrix.niter)
        self.opq_niter_pq = 4        # Lloyd iterations per outer iteration after the first (faiss OPQMatrix.niter_pq)
        self.rotation: Optional[torch.Tensor] = None      # [d, d] fp32, orthonormal: y = R r

    @property
    def is_trained(self) -> bool:
        return super().is_trained and self.rotation is not None

    def hbm_bytes(self) -> int:
        return super().hbm_bytes() + self.rotation.numel() * self.rotation.element_size()

    def set_rotation(self, rotation) -> None:
        """Install a trained rotation [d, d] (file load, the sharded build's broadcast, tests)."""
        r = _as_tensor(rotation, np.float32)
        if tuple(r.shape) != (self.d, self.d):
            raise ValueError(f"set_rotation: expected [{self.d},{self.d}]")
        self.rotation = r.to(self.device, torch.float32).contiguous()

    def state_host(self) -> dict:
        return dict(super().state_host(), rotation=self.rotation.cpu().numpy())

    def _rotate(self, x: torch.Tensor, rotation: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [n, d] R^T: row i becomes R x_i (wise_opq_rotate)."""
        r = self.rotation if rotation is None else rotation
        out = torch.empty_like(x)
        _lib.check(_lib.lib().wise_opq_rotate(x.data_ptr(), r.data_ptr(), x.shape[0], self.d, out.data_ptr(), _lib.stream_ptr()),
                   "wise_opq_rotate")
        return out

    def _code_input(self, xs: torch.Tensor, assign: torch.Tensor) -> torch.Tensor:
        return self._rotate(self._residuals(xs, assign))

    def _table_queries(self, qs: torch.Tensor) -> torch.Tensor:
        return self._rotate(qs)

    def _correlation(self, codes: torch.Tensor, codebooks: torch.Tensor, resid: torch.Tensor) -> np.ndarray:
        """M = sum_i cw_i x_i^T [d, d] float64 on the host (wise_opq_corr): cw_i the codewords of row i, x_i its unrotated residual."""
        lib = _lib.lib()
        n = resid.shape[0]
        M = torch.empty(self.d, self.d, dtype=torch.float64, device=self.device)
        ws = self._workspace(lib.wise_opq_corr_workspace_bytes(n, self.d))
        _lib.check(lib.wise_opq_corr(codes.data_ptr(), codebooks.data_ptr(), resid.data_ptr(), n, self.d, self.m, M.data_ptr(),
                                     ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "wise_opq_corr")
        return M.cpu().numpy()

    def train_rotation(self, resid: torch.Tensor):
        """(rotation [d, d], codebooks [m, 256, dsub]) from the training residuals: from R = I, opq_niter times {rotate, fit the
        codebooks, encode, M = sum cw x^T, R = U V^T of M's SVD}, then one more rotation and fit.  The first fit is
        train_codebooks as IVFPQIPIndex runs it (R = I: iteration 0 is plain PQ); the later ones are opq_niter_pq Lloyd
        iterations from the codebooks they find.  The SVD is numpy's, in float64 on the host."""
        rot = torch.eye(self.d, dtype=torch.float32, device=self.device)
        cb = None
        for t in range(max(int(self.opq_niter), 1)):
            xr = self._rotate(resid, rot)
            if cb is None:
                cb = self.train_codebooks(xr)
            else:
                for _ in range(self.opq_niter_pq):
                    cb = self._update(xr, self._encode(xr, cb), cb)
            u, _, vt = np.linalg.svd(self._correlation(self._encode(xr, cb), cb, resid))
            rot = torch.from_numpy(np.ascontiguousarray((u @ vt).astype(np.float32))).to(self.device)
        xr = self._rotate(resid, rot)
        for _ in range(self.opq_niter_pq):
            cb = self._update(xr, self._encode(xr, cb), cb)
        return rot, cb

    def train(self, x) -> None:
        x = _rows_f32(x, self.d, "train")
        if x.shape[0] < KSUB:
            raise ValueError(f"train: {x.shape[0]} training vectors for {KSUB} codewords")
        self._coarse.train(x)
        x = x.to(self.device, torch.float32).contiguous()
        self.rotation, self.codebooks = self.train_rotation(self.training_residuals(x))


class IVFOPQIPIndex(_OPQRotation, IVFPQIPIndex):
    """IVFPQIPIndex behind a learned rotation (index types IndexIVFOPQ<m>; module docstring)."""

    def __init__(self, d: int, nlist: int, m: int, nbits: int = 8, device: str = "cuda"):
        check_opq_shape(int(d), int(m))
        super().__init__(d, nlist, m, nbits, device)
        self._init_rotation()

    def reconstruct_batch(self, ids) -> np.ndarray:
        """Decoded rows with the rotation undone: c_l + R^T concat_j cb[j][code_j]; NaN for an unknown id."""
        lib = _lib.lib()
        pos = self._positions(ids)
        st, ls = _lib.stream_ptr(), self._lists
        out = torch.empty(pos.numel(), self.d, dtype=torch.float32, device=self.device)
        _lib.check(lib.wise_opq_decode(ls.data.data_ptr(), ls.n, pos.data_ptr(), pos.numel(), ls.list_off.data_ptr(), self.nlist,
                                       self.centroids.data_ptr(), self.codebooks.data_ptr(), self.rotation.data_ptr(), self.d, self.m,
                                       out.data_ptr(), st), "wise_opq_decode")
        return out.cpu().numpy()


class IVFOPQRefineIPIndex(_OPQRotation, IVFPQRefineIPIndex):
    """IVFPQRefineIPIndex behind a learned rotation (index types IndexIVFOPQ<m>R8 / R16): the codes come from the rotated
    residuals, the compact rows and the re-ranking stage from the rows and queries as they are."""

    def __init__(self, d: int, nlist: int, m: int, kind: int, k_factor: int = DEFAULT_K_FACTOR, device: str = "cuda"):
        check_opq_shape(int(d), int(m))
        super().__init__(d, nlist, m, kind, k_factor, device)
        self._init_rotation()

"""faiss-shaped inverted-file index (inner product) whose lists live in HBM and whose search is two HIP scans.

Stands where `faiss.IndexIVFFlat(IndexFlatIP(d), d, nlist, METRIC_INNER_PRODUCT)` stands in the reference
(src/index/feature_search_index.py:53-76: nlist = 3 or 10 * round(sqrt(N)), trained on min(N, 100 * nlist) rows;
api/routes.py:899-909 then sets `parallel_mode`, `nprobe` and calls `make_direct_map(True)`).

  train(x)            spherical k-means (10 Lloyd iterations, assignment by inner product — what faiss's Clustering
                      does for an inner-product IVF), run on the GPU as dense products; deterministic (seeded
                      sample for the initial centroids, empty cells re-seeded from the fullest cell)
  add_with_ids(x,ids) rows are assigned to the centroid of largest inner product and kept grouped by list
  search(q, k)        stage 1: `nprobe` best centroids per query = wise_ip_topk_f32 over the centroid table (nprobe
                      <= 64) or wise_ip_scores_f32 + wise_select_topk_f32 (the reference's nprobe = 1024);
                      stage 2: wise_ivf_scan_f32 over the probed lists (the flat scan kernel run per list segment)
The quantizer (train, assign, probes) and the list bookkeeping are ivf_common.py's CoarseQuantizer and ListStore, shared
with ivf_pq.py; this file keeps the flat scan.
An approximate index cannot be pinned value-for-value against faiss (its k-means starts from faiss's own random
permutation); what IS exact and tested: given the same centroids and lists, the result equals the brute-force top-k
restricted to the probed lists (oracle/ivf_ref.py), and nprobe = nlist reproduces the flat index.

IVFFlatL2Index (index type 'IndexIVFFlatL2') is the same index under squared L2 — `faiss.IndexIVFFlat(IndexFlatL2(d), d, nlist,
METRIC_L2)` — for rows whose length carries meaning.  The lists hold the raw fp32 rows (no residual).  What differs:
  train(x)            plain k-means (ivf_common.py: L2CoarseQuantizer), centroids are means, not unit vectors
  coarse rule         g(x, c) = fl(x . c - |c|^2 / 2) (wise_ip_scores_f32, wise_ivf_l2_coarse), argmax for a row's list
                      (wise_ivf_argmax), the nprobe largest for a query's probes (wise_select_topk_f32): one path at every nprobe
  search(q, k)        wise_ivfl2_scan over the probed lists: a row's distance is, bit for bit, IndexFlatL2's for the same (query,
                      row); squared distances, ascending, padded with (+3.4028235e38, -1); range hit: dist < thresh, strictly
  limits              IndexFlatL2's: d % 16 == 0 in [16, 1024]
tests/ivf_l2_ref.py restates all of it; nprobe = nlist reproduces FlatL2Index's distances bit for bit.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from .. import _lib
from .ivf_common import CoarseQuantizer, IVFIndexBase, L2CoarseQuantizer, _DirectMap, _ids_i64, _rows_f32  # noqa: F401  (_DirectMap: re-exported)


def reference_nlist(feature_count: int) -> int:
    """The cell count the reference picks (feature_search_index.py:55-58)."""
    return (3 if feature_count < 200000 else 10) * round(math.sqrt(feature_count))


class IVFFlatIPIndex(IVFIndexBase):
    GROUP_SCORES = "wise_ivf_group_scores_f32"

    def __init__(self, d: int, nlist: int, device: str = "cuda"):
        super().__init__(d, nlist, device, width=int(d), dtype=torch.float32, gather=CoarseQuantizer._gather_rows)

    niter = property(lambda self: self._coarse.niter, lambda self, v: setattr(self._coarse, "niter", v))
    seed = property(lambda self: self._coarse.seed, lambda self, v: setattr(self._coarse, "seed", v))

    def train(self, x) -> None:
        self._coarse.train(x)

    def assign(self, x, chunk: int = 1 << 20) -> np.ndarray:
        return self._coarse.assign(x, chunk)

    # -- construction ---------------------------------------------------------------------------
    def add_with_ids(self, x, ids) -> None:
        if not self.is_trained:
            raise RuntimeError(f"{type(self).__name__}: train() before add_with_ids()")
        x = _rows_f32(x, self.d, "add_with_ids")
        ids = _ids_i64(ids, x.shape[0])
        x = x.to(self.device, torch.float32).contiguous()
        ids = ids.to(self.device, torch.int64).contiguous()
        self._lists.append(x, ids, self._coarse.assign_device(x, self.centroids))

    def adopt_lists(self, X: torch.Tensor, ids: torch.Tensor, list_off: torch.Tensor) -> "IVFFlatIPIndex":
        """Take rows that are already grouped by list (file load)."""
        self._lists.adopt(X, ids, list_off)
        return self

    # -- search ---------------------------------------------------------------------------------
    def _scan(self, q: torch.Tensor, k: int, local: bool, probe_count: Optional[torch.Tensor], sel=None):
        """stage 1 + stage 2.  local: wise_ivf_scan_local_f32, which drops the probes whose segment is empty in this
        index before it scans and merges, and reports the number kept per query in `probe_count` when given.
        sel: an IDSelector — wise_ivf_scan_sel_f32 over the same probes, only the selected rows compete."""
        lib = _lib.lib()
        q = self._queries(q)
        keep = self._keep(sel)
        if keep is not None and local:
            raise NotImplementedError("IVFFlatIPIndex: a rank's share of a search takes no selector")
        nq = q.shape[0]
        D = torch.empty(nq, k, dtype=torch.float32, device=self.device)
        I = torch.empty(nq, k, dtype=torch.int64, device=self.device)
        if nq == 0:
            return D, I
        nprobe = self._clamped_nprobe()
        probes = self._coarse.probes_device(q, nprobe).contiguous()
        need = (lib.wise_ivf_scan_local_workspace_bytes if local else lib.wise_ivf_scan_workspace_bytes)(nq, nprobe, k)
        if need == 0:
            raise ValueError(f"search: unsupported shape nq={nq} nprobe={nprobe} k={k}")
        ws, ls = self._workspace(need), self._lists
        if probe_count is not None and (probe_count.dtype != torch.int32 or probe_count.numel() < nq
                                        or probe_count.device != ws.device):
            raise ValueError("search_local_device: probe_count must be an int32 device tensor of nq entries")
        head = (ls.data.data_ptr(), ls.n, self.d, ls.list_off.data_ptr(), self.nlist, ls.ids.data_ptr(), q.data_ptr(), nq,
                probes.data_ptr(), nprobe, k, D.data_ptr(), I.data_ptr())
        tail = (ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        if keep is not None:
            _lib.check(lib.wise_ivf_scan_sel_f32(*head[:11], keep.data_ptr(), *head[11:], *tail), "wise_ivf_scan_sel_f32")
        elif local:
            _lib.check(lib.wise_ivf_scan_local_f32(*head, _lib.ptr(probe_count), *tail), "wise_ivf_scan_local_f32")
        else:
            _lib.check(lib.wise_ivf_scan_f32(*head, *tail), "wise_ivf_scan_f32")
        return D, I

    def search_device(self, q: torch.Tensor, k: int, sel=None):
        return self._scan(q, k, False, None, sel)

    def search_local_device(self, q: torch.Tensor, k: int, probe_count: Optional[torch.Tensor] = None):
        """search_device for an index that holds ONE RANK's slice of a list-major index sharded across GPUs (its
        list_off clipped to the slice; ShardedIVFFlatIPIndex): the same coarse stage over the full centroid table,
        then the local scan.  probe_count: optional [nq] int32 device tensor that receives the number of probes kept
        per query."""
        return self._scan(q, k, True, probe_count)

    def _range_workspace_bytes(self, nq: int, nprobe: int) -> int:
        return _lib.lib().wise_ivf_range_workspace_bytes(self._lists.n, self.nlist, nq, nprobe)

    def _range_stage(self, qs, probes, nprobe, radius, keep):
        lib, ls, st, n = _lib.lib(), self._lists, _lib.stream_ptr(), qs.shape[0]
        head = (ls.data.data_ptr(), ls.n, self.d, ls.list_off.data_ptr(), self.nlist)

        def count(counts, ws):
            _lib.check(lib.wise_ivf_range_count_f32(*head, qs.data_ptr(), n, probes.data_ptr(), nprobe, radius, _lib.ptr(keep),
                                                    counts.data_ptr(), ws.data_ptr(), ws.numel(), st), "wise_ivf_range_count_f32")

        def fill(lims, D, P, ws):
            _lib.check(lib.wise_ivf_range_fill_f32(*head, 0, qs.data_ptr(), n, probes.data_ptr(), nprobe, radius, lims.data_ptr(),
                                                   D.data_ptr(), P.data_ptr(), ws.data_ptr(), ws.numel(), st), "wise_ivf_range_fill_f32")
        return count, fill

    # -- the rest of the surface the REST layer touches -------------------------------------------
    def reconstruct_batch(self, ids) -> np.ndarray:
        lib = _lib.lib()
        self._finalize()
        ls = self._lists
        qi = torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int64)).to(self.device)
        out = torch.empty(qi.numel(), self.d, dtype=torch.float32, device=self.device)
        rc = lib.wise_reconstruct_batch(ls.data.data_ptr(), ls.n, self.d, ls.ids.data_ptr(), 0, qi.data_ptr(),
                                        qi.numel(), out.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "wise_reconstruct_batch")
        return out.cpu().numpy()

    def lists_host(self):
        """(centroids [nlist,d], X [N,d], ids [N], list_off [nlist+1]) as numpy (file save, tests)."""
        self._finalize()
        ls = self._lists
        return self.centroids.cpu().numpy(), ls.data.cpu().numpy(), ls.ids.cpu().numpy(), ls.list_off.cpu().numpy()

    def state_host(self) -> dict:
        """The index as the dict faiss_io.read_ivf_flat_ip returns and faiss_io.write_index takes."""
        return dict(zip(("centroids", "X", "ids", "list_off"), self.lists_host()), nprobe=self.nprobe)


def check_l2_shape(d: int) -> None:
    """The shapes wise_ivfl2_* serve (include/wise_hip.h: IndexFlatL2's); ValueError otherwise."""
    if d < 16 or d % 16 != 0 or d > 1024:
        raise ValueError(f"IndexIVFFlatL2: d={d} must be a multiple of 16 in [16, 1024] (a row is read in 16-byte loads)")


class IVFFlatL2Index(IVFFlatIPIndex):
    """Index type 'IndexIVFFlatL2' (module docstring).  Everything that does not look at the metric — the list store, chunked adds,
    the direct map, reconstruct_batch, remove_ids, the selector plumbing — is IVFFlatIPIndex's.  Across GPUs an index holds one
    rank's slice of the list-major rows: list_off clipped to the slice and `pos_base`, the position of its first row."""
    COARSE = L2CoarseQuantizer
    metric = "l2"
    GROUP_SCORES = "wise_ivfl2_group_scores"

    def __init__(self, d: int, nlist: int, device: str = "cuda"):
        check_l2_shape(int(d))
        super().__init__(d, nlist, device)
        self.pos_base = 0

    def adopt_lists(self, X: torch.Tensor, ids: torch.Tensor, list_off: torch.Tensor, pos_base: int = 0) -> "IVFFlatL2Index":
        """Take rows that are already grouped by list (file load).  pos_base: the rows are a slice of a larger list-major array
        that starts at this position of it (list_off clipped to the slice)."""
        if X.dim() != 2 or X.shape[1] != self.d:
            raise ValueError(f"adopt_lists: expected rows [n,{self.d}]")
        if pos_base < 0:
            raise ValueError("adopt_lists: pos_base must not be negative")
        self._lists.adopt(X, ids, list_off)
        self.pos_base = int(pos_base)
        return self

    # -- search ---------------------------------------------------------------------------------
    def _scan(self, q: torch.Tensor, k: int, local: bool, probe_count: Optional[torch.Tensor], sel=None, positions: bool = False):
        """The coarse rule, then wise_ivfl2_scan; sel: wise_ivfl2_scan_sel over the same probes; local: wise_ivfl2_scan_local (the
        probes whose list is empty in this slice dropped first, their number to probe_count when given).  positions: I receives
        positions in the lists (local: in the WHOLE array) instead of external ids."""
        lib = _lib.lib()
        q = self._queries(q)
        keep = self._keep(sel)
        if keep is not None and local:
            raise NotImplementedError("IVFFlatL2Index: a rank's share of a search takes no selector")
        nq, k = q.shape[0], int(k)
        D = torch.empty(nq, k, dtype=torch.float32, device=self.device)
        I = torch.empty(nq, k, dtype=torch.int64, device=self.device)
        if nq == 0:
            return D, I
        if probe_count is not None and (probe_count.dtype != torch.int32 or probe_count.numel() < nq or probe_count.device != q.device
                                        or not probe_count.is_contiguous()):
            raise ValueError("search_local_device: probe_count must be a contiguous int32 device tensor of nq entries")
        nprobe = self._clamped_nprobe()
        probes = self._coarse.probes_device(q, nprobe)
        need = (lib.wise_ivfl2_scan_local_workspace_bytes if local else lib.wise_ivfl2_scan_workspace_bytes)(nq, nprobe, k)
        if need == 0:
            raise ValueError(f"search: unsupported shape nq={nq} nprobe={nprobe} k={k}")
        ws, ls = self._workspace(need), self._lists
        head = (ls.data.data_ptr(), ls.n, self.d, ls.list_off.data_ptr(), self.nlist, 0 if positions else ls.ids.data_ptr(), q.data_ptr(),
                nq, probes.data_ptr(), nprobe, k)
        out = (D.data_ptr(), I.data_ptr())
        tail = (ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        if local:
            _lib.check(lib.wise_ivfl2_scan_local(*head, self.pos_base, *out, _lib.ptr(probe_count), *tail), "wise_ivfl2_scan_local")
        elif keep is not None:
            _lib.check(lib.wise_ivfl2_scan_sel(*head, keep.data_ptr(), *out, *tail), "wise_ivfl2_scan_sel")
        else:
            _lib.check(lib.wise_ivfl2_scan(*head, *out, *tail), "wise_ivfl2_scan")
        return D, I

    def search_local_device(self, q: torch.Tensor, k: int, probe_count: Optional[torch.Tensor] = None, positions: bool = False):
        """search_device for an index that holds ONE RANK's slice (adopt_lists with pos_base; ShardedIVFFlatIPIndex): the same coarse
        stage over the full centroid table, then the local scan.  wise_topk_merge of the ranks' negated answers in rank order gives
        the one-GPU answer's bits."""
        return self._scan(q, k, True, probe_count, positions=positions)

    def _range_workspace_bytes(self, nq: int, nprobe: int) -> int:
        return _lib.lib().wise_ivfl2_range_workspace_bytes(self._lists.n, self.nlist, nq, nprobe)

    def _range_stage(self, qs, probes, nprobe, radius, keep):
        lib, ls, st, n = _lib.lib(), self._lists, _lib.stream_ptr(), qs.shape[0]
        head = (ls.data.data_ptr(), ls.n, self.d, ls.list_off.data_ptr(), self.nlist)

        def count(counts, ws):
            _lib.check(lib.wise_ivfl2_range_count(*head, qs.data_ptr(), n, probes.data_ptr(), nprobe, radius, _lib.ptr(keep),
                                                  counts.data_ptr(), ws.data_ptr(), ws.numel(), st), "wise_ivfl2_range_count")

        def fill(lims, D, P, ws):
            _lib.check(lib.wise_ivfl2_range_fill(*head, 0, qs.data_ptr(), n, probes.data_ptr(), nprobe, radius, lims.data_ptr(),
                                                 D.data_ptr(), P.data_ptr(), ws.data_ptr(), ws.numel(), st), "wise_ivfl2_range_fill")
        return count, fill

    def state_host(self) -> dict:
        """The index as the dict faiss_io.read_ivf_flat_l2 returns and faiss_io.write_index takes: IVFFlatIPIndex's and metric='l2'."""
        return dict(super().state_host(), metric="l2")

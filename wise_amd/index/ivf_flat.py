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
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from .. import _lib
from .ivf_common import CoarseQuantizer, IVFIndexBase, _DirectMap, _ids_i64, _rows_f32  # noqa: F401  (_DirectMap: re-exported)


def reference_nlist(feature_count: int) -> int:
    """The cell count the reference picks (feature_search_index.py:55-58)."""
    return (3 if feature_count < 200000 else 10) * round(math.sqrt(feature_count))


class IVFFlatIPIndex(IVFIndexBase):
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
            raise RuntimeError("IVFFlatIPIndex: train() before add_with_ids()")
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

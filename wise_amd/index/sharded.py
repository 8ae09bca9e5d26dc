"""Row-sharded flat IP index: one process per GPU, each rank owns a contiguous slice of the rows.

Per query batch: local HIP scan+top-k on every rank -> ONE all-gather of the per-shard
(score, id)[nq,k] lists packed in one int64 buffer (RCCL over xGMI; 16*nq*k bytes per rank, latency-bound) -> the
same k-way merge kernel on every rank, so every rank returns the global result.
The reference has no distributed path; this is the only collective the search needs.

ShardedIVFFlatIPIndex does the same for IndexIVFFlat.  The index is one list-major array (list 0's rows, then list 1's,
...) and rank r owns rows shard_range(N, r, W) of it; every rank keeps the whole centroid table and list_off clipped to
its range (a list that straddles a boundary is split, head on the lower rank).  The coarse stage runs on every rank,
the list scan only over the probed lists the rank holds (wise_ivf_scan_local_f32: ~nprobe / W of them), then the same
exchange and merge.  A rank's rows are in global order and the merge puts the lower rank first on equal scores, so the
answer has the bits of the one-GPU IVF search over the same centroids and lists, ties included.

ShardedIVFPQIPIndex is that wrapper around a slice of an IndexIVFPQ<m> (codes instead of rows, all codebooks on every rank,
wise_ivfpq_scan_local): one exchange.  ShardedIVFPQRefineIPIndex (IndexIVFPQ<m>R8 / R16) needs TWO exchanges to return the
one-GPU answer, because the one-GPU index re-ranks the kc best positions of the WHOLE PQ scan: (1) every rank's kc best
positions are gathered and merged into those global kc, (2) every rank re-ranks the ones that lie in its slice
(wise_ivf_refine_local) and the ranks' k best are gathered and merged.  Re-ranking each rank's own kc would save a collective
and return a different answer (a pool of W * kc).

ShardedIVFSQIPIndex wraps a slice of an IndexIVFSQ8 (d code bytes per row, the centroids and the [2 d] ranges on every rank,
wise_ivfsq_scan_local): one exchange, as ShardedIVFPQIPIndex.  reconstruct_batch is the flat wrapper's: the rank that holds an id
decodes it (wise_sq_decode against its clipped offsets), the others answer NaN.  ShardedIVFSQfp16IPIndex is the same wrapper around
a slice of an IndexIVFSQfp16 (2 d bytes per row, only the centroids replicated, wise_ivfsq16_scan_local).
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import torch
import torch.distributed as dist

from .. import _lib
from .flat_common import FlatIndexBase
from .selector import unpack_params


def shard_range(n_total: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous rows [lo, hi) of rank `rank`; sizes differ by at most one row."""
    if not (0 <= rank < world):
        raise ValueError(f"rank {rank} outside world {world}")
    return (n_total * rank) // world, (n_total * (rank + 1)) // world


def merge_device(Ds: torch.Tensor, Is: torch.Tensor, k: int):
    """[parts,nq,k] device tensors -> [nq,k] via wise_topk_merge."""
    lib = _lib.lib()
    parts, nq, kk = Ds.shape
    D = torch.empty(nq, k, dtype=torch.float32, device=Ds.device)
    I = torch.empty(nq, k, dtype=torch.int64, device=Ds.device)
    _lib.check(lib.wise_topk_merge(Ds.contiguous().data_ptr(), Is.contiguous().data_ptr(), parts, nq, kk,
                                   D.data_ptr(), I.data_ptr(), _lib.stream_ptr()), "wise_topk_merge")
    return D, I


NO_SELECTOR = ("the sharded indexes take no selector: a collective filtered search is not built (each rank would resolve the "
               "selector against its own ids and the exchange would stay as it is); search the ranks' local indexes or an "
               "unsharded index instead")


NO_COLLECTIVE_REMOVAL = ("the sharded indexes have no remove_ids: a collective removal is not built (every rank would compact its "
                         "slice and the slices' row ranges would have to be agreed on again); remove from the unsharded index "
                         "and shard it again")


class ShardedFlatIPIndex:
    """Every rank constructs it around its own local FlatIPIndex, FlatSQfp16IPIndex or FlatL2Index (rows [lo,hi) of the global
    index, ids already global).  `search_device` is collective: all ranks call it with the same queries."""

    def __init__(self, local: FlatIndexBase, group: Optional[dist.ProcessGroup] = None,
                 local_search: Optional[Callable] = None, merge: Optional[Callable] = None,
                 always_exchange: bool = False):
        """always_exchange: run the all-gather and the merge even when the group has ONE rank (the collective and the
        merge kernel can then be exercised on a one-GPU box: tests/test_gpu_sharded.py)."""
        self.local = local
        self.group = group
        self.d = local.d
        self.always_exchange = bool(always_exchange)
        # injection points exist for the CPU (gloo) tests only; the product path is the HIP one
        self._local_search = local_search or local.search_device
        self._merge = merge or merge_device
        self._xchg = {}
        self.last_exchange_bytes = 0    # payload this rank contributed to the all-gather(s) of the last search

    @property
    def world(self) -> int:
        return dist.get_world_size(self.group) if dist.is_initialized() else 1

    @property
    def ntotal(self) -> int:
        n = torch.tensor([self.local.ntotal], dtype=torch.int64,
                         device=self.local.device if dist.is_initialized() and dist.get_backend(self.group) == "nccl"
                         else "cpu")
        if dist.is_initialized() and (self.world > 1 or self.always_exchange):
            dist.all_reduce(n, group=self.group)
        return int(n.item())

    def _exchanges(self) -> bool:
        return dist.is_initialized() and (self.world > 1 or self.always_exchange)

    def search_device(self, q: torch.Tensor, k: int, sel=None):
        if sel is not None:
            raise NotImplementedError(NO_SELECTOR)
        D, I = self._local_search(q, k)
        if not self._exchanges():
            return D, I
        self.last_exchange_bytes = 0
        if getattr(self.local, "metric", "ip") == "l2":
            # the exchange and the merge keep the larger score: they run on the negated distances (exact; the local padding
            # +3.4028235e38 travels as the merge's own -3.4028235e38) and the sign flips back on the result
            D, I = self._exchange_merge(-D, I, k)
            return -D, I
        return self._exchange_merge(D, I, k)

    def _exchange_merge(self, D: torch.Tensor, I: torch.Tensor, k: int):
        """All-gather of every rank's (D, I) [nq, k] and the merge in rank order; adds to last_exchange_bytes."""
        W = self.world
        nq = D.shape[0]
        # ONE collective per query batch: scores and ids travel as one int64 buffer per rank — plane 0 the fp32 score
        # bits (as int32 values), plane 1 the ids — 16 * nq * k bytes (160 B at nq = 1, k = 10).  The exchange is
        # latency-bound (at 8 ranks the local scan of a 10M-row index is ~0.2 ms), so the number of collectives is what
        # counts, not their payload.  Buffers are kept between calls.
        key = (nq, k, D.device)
        if key not in self._xchg:
            if len(self._xchg) >= 4:
                self._xchg.clear()
            self._xchg[key] = (torch.empty(2, nq, k, dtype=torch.int64, device=D.device),
                               torch.empty(W, 2, nq, k, dtype=torch.int64, device=D.device))
        send, recv = self._xchg[key]
        send[0].copy_(D.contiguous().view(torch.int32))        # exact: int32 -> int64 and back keeps the float's bits
        send[1].copy_(I)
        dist.all_gather_into_tensor(recv.view(W * 2 * nq, k), send.view(2 * nq, k), group=self.group)
        Ds = recv[:, 0].to(torch.int32).view(torch.float32)
        Is = recv[:, 1].contiguous()
        self.last_exchange_bytes += send.numel() * 8
        return self._merge(Ds, Is, k)

    def search(self, x, k: int, params=None):
        """faiss signature, collective: every rank calls it with the same x and gets the global result.
        params: a selector is refused (NotImplementedError); SearchParametersIVF(nprobe=...) holds for this call only."""
        import numpy as np

        sel, nprobe = unpack_params(params, ivf=hasattr(self.local, "nprobe"))
        if sel is not None:
            raise NotImplementedError(NO_SELECTOR)
        q = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.local.device)
        kept = getattr(self.local, "nprobe", None)
        try:
            if nprobe is not None:
                self.local.nprobe = nprobe
            D, I = self.search_device(q, int(k))
        finally:
            if nprobe is not None:
                self.local.nprobe = kept
        return D.cpu().numpy(), I.cpu().numpy()

    def range_search(self, x, thresh: float, params=None):
        """Not built: the result is variable-length and nothing exchanges it between the ranks."""
        from .range_search import NO_SHARDED
        raise NotImplementedError(NO_SHARDED)

    range_search_device = range_search

    def search_grouped(self, *args, **kwargs):
        """Not built: a group's rows may lie on several ranks and nothing exchanges per-group representatives."""
        from .group_search import NO_SHARDED as NO_SHARDED_GROUPS
        raise NotImplementedError(NO_SHARDED_GROUPS)

    search_grouped_device = set_groups = search_grouped

    def remove_ids(self, sel, scratch_bytes=None) -> int:
        """Not built: every rank would have to compact its slice and the ranks agree on the new row ranges."""
        raise NotImplementedError(NO_COLLECTIVE_REMOVAL)

    def reconstruct_batch(self, ids):
        """IndexIDMap::reconstruct_batch over the shards (api/routes.py:1078), collective: every rank looks the ids up in
        its own rows (a row of NaN where it does not hold the id — wise_reconstruct_batch), ONE all-gather of the [n,d]
        answers, and each row is taken from the rank that had it.  Ids no rank holds stay NaN."""
        import numpy as np

        mine = torch.from_numpy(np.ascontiguousarray(self.local.reconstruct_batch(ids), dtype=np.float32))
        if not dist.is_initialized() or (self.world == 1 and not self.always_exchange):
            return mine.numpy()
        W = self.world
        on_device = dist.get_backend(self.group) == "nccl"
        mine = mine.to(self.local.device) if on_device else mine
        allr = torch.empty((W,) + tuple(mine.shape), dtype=torch.float32, device=mine.device)
        dist.all_gather_into_tensor(allr.view(W * mine.shape[0], -1), mine, group=self.group)
        have = ~torch.isnan(allr[:, :, 0])                        # [W, n]
        owner = have.to(torch.int8).argmax(dim=0)                 # first rank that holds the id (ids are unique)
        out = allr[owner, torch.arange(mine.shape[0], device=mine.device)]
        return out.cpu().numpy()


class ShardedIVFFlatIPIndex(ShardedFlatIPIndex):
    """Every rank constructs it around its own local IVFFlatIPIndex holding a clipped slice of the list-major array
    (full centroid table, ids global).  search_device / ntotal / reconstruct_batch are collective as in the flat
    wrapper; the rest is the surface api/routes.py:899-909 touches, passed on to the local index."""

    def __init__(self, local, group: Optional[dist.ProcessGroup] = None, local_search: Optional[Callable] = None,
                 merge: Optional[Callable] = None, always_exchange: bool = False):
        super().__init__(local, group=group, local_search=local_search or local.search_local_device, merge=merge,
                         always_exchange=always_exchange)

    @property
    def nprobe(self) -> int:
        return self.local.nprobe

    @nprobe.setter
    def nprobe(self, v: int) -> None:
        self.local.nprobe = int(v)

    @property
    def parallel_mode(self) -> int:
        return self.local.parallel_mode

    @parallel_mode.setter
    def parallel_mode(self, v: int) -> None:
        self.local.parallel_mode = v

    @property
    def direct_map(self):
        return self.local.direct_map

    @property
    def is_trained(self) -> bool:
        return self.local.is_trained

    @property
    def nlist(self) -> int:
        return self.local.nlist

    def make_direct_map(self, enable: bool = True) -> None:
        self.local.make_direct_map(enable)


class ShardedIVFPQIPIndex(ShardedIVFFlatIPIndex):
    """Every rank constructs it around its own local IVFPQIPIndex holding a clipped slice of the list-major codes (all
    centroids and codebooks, ids global, `pos_base` set).  One exchange per search, the flat wrapper's."""

    @property
    def is_trained(self) -> bool:
        return self.local.is_trained

    def hbm_bytes(self) -> int:
        """Of this rank's slice (local, not collective)."""
        return self.local.hbm_bytes()


class ShardedIVFSQIPIndex(ShardedIVFFlatIPIndex):
    """Every rank constructs it around its own local IVFSQIPIndex holding a clipped slice of the list-major codes (all
    centroids and the ranges, ids global, `pos_base` set).  One exchange per search, the flat wrapper's."""

    def hbm_bytes(self) -> int:
        """Of this rank's slice (local, not collective)."""
        return self.local.hbm_bytes()


class ShardedIVFSQfp16IPIndex(ShardedIVFSQIPIndex):
    """Around a local IVFSQfp16IPIndex slice (binary16 rows, all centroids, ids global, `pos_base` set): nothing differs."""


MAX_MERGE_KEYS = 65536           # wise_topk_merge: parts * k


class ShardedIVFPQRefineIPIndex(ShardedIVFPQIPIndex):
    """Around a local IVFPQRefineIPIndex slice.  Two exchanges per search (module docstring): the candidates, then the
    re-ranked answers; last_exchange_bytes is the sum, 16 * nq * (candidates(k) + k) bytes per rank."""

    def __init__(self, local, group: Optional[dist.ProcessGroup] = None, merge: Optional[Callable] = None,
                 always_exchange: bool = False):
        super().__init__(local, group=group, local_search=local.search_device, merge=merge, always_exchange=always_exchange)

    @property
    def k_factor(self) -> int:
        return self.local.k_factor

    @k_factor.setter
    def k_factor(self, v: int) -> None:
        self.local.k_factor = int(v)

    def search_device(self, q: torch.Tensor, k: int, sel=None):
        if sel is not None:
            raise NotImplementedError(NO_SELECTOR)
        if not self._exchanges():
            return self.local.search_device(q, k)
        kc = self.local.candidates(k)
        if self.world * kc > MAX_MERGE_KEYS:
            raise ValueError(f"ShardedIVFPQRefineIPIndex: {self.world} ranks x {kc} candidates exceed the {MAX_MERGE_KEYS} keys one "
                             f"merge takes (at most {MAX_MERGE_KEYS // kc} ranks at k = {k}, k_factor = {self.local.k_factor})")
        self.last_exchange_bytes = 0
        cD, cP = self.local.candidates_local_device(q, kc)
        _, cand = self._exchange_merge(cD, cP, kc)                   # the kc positions the one-GPU PQ scan returns
        D, I = self.local.refine_local_device(q, cand, k)
        return self._exchange_merge(D, I, k)

"""What the inverted-file indexes (ivf_flat.py, ivf_sq.py, ivf_pq.py) are made of: one coarse quantizer, one list store, and
the faiss-shaped surface around the two.

  CoarseQuantizer     the centroid table and everything that uses it: spherical k-means (10 Lloyd iterations, assignment
                      by inner product — what faiss's Clustering does for an inner-product IVF), run on the GPU as dense
                      products; deterministic (seeded sample for the initial centroids, empty cells re-seeded from the
                      fullest cell); the assignment of rows to lists; the probes of a query
  L2CoarseQuantizer   the same for the L2 metric (IndexIVFFlatL2): plain k-means and the coarse rule s(x, c) - |c|^2 / 2, one path
                      for assignment and probes
  ListStore           the payload (fp32 rows or uint8 codes) and the ids grouped by list, with the chunks added since the
                      last merge; optionally further per-row arrays kept in the same order (the compact rows a re-ranking
                      index scores its candidates from, ivf_pq.py)
  IVFIndexBase        nprobe, direct map, numpy search and the other attributes the REST layer touches on either index
  CodedIVFIndexBase   the indexes whose lists hold encoded residuals (ivf_sq.py, ivf_pq.py): add_with_ids, encode_rows,
                      adopt_lists with pos_base, the one-stage search with its selector and rank-local forms, id lookup
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from .. import _lib
from . import group_search as _group
from . import mutate as _mutate
from . import range_search as _range
from .flat_ip import FlatIPIndex
from .selector import resolve_for, unpack_params


def _as_tensor(x, dtype) -> torch.Tensor:
    """A tensor is passed through as it is; anything else becomes a contiguous host tensor of the numpy `dtype`."""
    return x if torch.is_tensor(x) else torch.as_tensor(np.ascontiguousarray(x, dtype=dtype))


def _rows_f32(x, d: int, what: str) -> torch.Tensor:
    x = _as_tensor(x, np.float32)
    if x.dim() != 2 or x.shape[1] != d:
        raise ValueError(f"{what}: expected [n,{d}], got {tuple(x.shape)}")
    return x


def _ids_i64(ids, n: int) -> torch.Tensor:
    ids = _as_tensor(ids, np.int64)
    if ids.shape != (n,):
        raise ValueError("add_with_ids: ids must have one entry per row")
    return ids


class _DirectMap:
    """The two attributes api/routes.py:1317 reads."""
    NoMap, Array, Hashtable = 0, 1, 2

    def __init__(self):
        self.type = self.NoMap


class CoarseQuantizer:
    # Everything numeric below is this library's own kernels (csrc/ivf_build.hip, wise_ip_scores_f32): torch only allocates,
    # concatenates and draws the seeding permutation on the host.
    def __init__(self, d: int, nlist: int, device: str = "cuda"):
        if d < 4 or d % 4 != 0 or d > 2048:
            raise ValueError(f"IVFFlatIPIndex: d={d} must be a multiple of 4 in [4, 2048]")
        if nlist < 1:
            raise ValueError("IVFFlatIPIndex: nlist must be positive")
        self.d, self.nlist = int(d), int(nlist)
        self.device = torch.device(device)
        self.is_trained = False
        self.niter = 10
        self.seed = 1234
        self.centroids: Optional[torch.Tensor] = None    # [nlist, d] fp32, unit rows
        self._quantizer: Optional[FlatIPIndex] = None

    @staticmethod
    def assign_device(x: torch.Tensor, centroids: torch.Tensor, chunk: int = 4096) -> torch.Tensor:
        """nearest centroid of every row by inner product: the exact-f32 score kernel (the coarse stage's own) + wise_ivf_argmax"""
        lib = _lib.lib()
        c = centroids.contiguous()
        out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
        scores = torch.empty(min(chunk, max(x.shape[0], 1)), c.shape[0], dtype=torch.float32, device=x.device)
        st = _lib.stream_ptr()
        for s in range(0, x.shape[0], chunk):
            q = x[s:s + chunk]                       # (a slice of whole rows of a contiguous tensor: contiguous)
            _lib.check(lib.wise_ip_scores_f32(c.data_ptr(), c.shape[0], c.shape[1], q.data_ptr(), q.shape[0],
                                              scores.data_ptr(), st), "wise_ip_scores_f32")
            _lib.check(lib.wise_ivf_argmax(scores.data_ptr(), q.shape[0], c.shape[0], out[s:].data_ptr(), st), "wise_ivf_argmax")
        return out

    def assign(self, x, chunk: int = 1 << 20) -> np.ndarray:
        """[n] int64 (numpy): the list each row of x [n,d] goes to (the assignment add_with_ids makes), streamed to the
        device `chunk` rows at a time."""
        if not self.is_trained:
            raise RuntimeError("IVFFlatIPIndex: train() before assign()")
        x = np.asarray(x, dtype=np.float32)
        out = np.empty(x.shape[0], dtype=np.int64)
        for s in range(0, x.shape[0], chunk):
            xs = torch.from_numpy(np.ascontiguousarray(x[s:s + chunk])).to(self.device)
            out[s:s + xs.shape[0]] = self.assign_device(xs, self.centroids).cpu().numpy()
        return out

    def _group(self, assign: torch.Tensor):
        """(order, list_off, counts): the rows grouped by list, stable (wise_ivf_group: a radix sort on the device)"""
        lib = _lib.lib()
        n = assign.shape[0]
        order = torch.empty(n, dtype=torch.int64, device=self.device)
        list_off = torch.empty(self.nlist + 1, dtype=torch.int64, device=self.device)
        counts = torch.empty(self.nlist, dtype=torch.int64, device=self.device)
        ws = torch.empty(lib.wise_ivf_group_workspace_bytes(n, self.nlist), dtype=torch.uint8, device=self.device)
        _lib.check(lib.wise_ivf_group(assign.data_ptr(), n, self.nlist, order.data_ptr(), list_off.data_ptr(), counts.data_ptr(),
                                      ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "wise_ivf_group")
        return order, list_off, counts

    @staticmethod
    def _gather_rows(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        out = torch.empty(idx.shape[0], x.shape[1], dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().wise_ivf_gather_rows(x.data_ptr(), idx.data_ptr(), idx.shape[0], x.shape[1], out.data_ptr(),
                                                   _lib.stream_ptr()), "wise_ivf_gather_rows")
        return out

    def train(self, x) -> None:
        lib = _lib.lib()  # raises without a gfx950 device: there is no CPU path
        x = _as_tensor(x, np.float32).to(self.device, torch.float32).contiguous()
        _rows_f32(x, self.d, "train")
        n = x.shape[0]
        if n < self.nlist:
            raise ValueError(f"train: {n} training vectors for {self.nlist} cells")
        st = _lib.stream_ptr()
        c = self._seed_rows(x)
        _lib.check(lib.wise_ivf_normalize_rows(c.data_ptr(), self.nlist, self.d, c.data_ptr(), st), "wise_ivf_normalize_rows")
        sums = torch.empty(self.nlist, self.d, dtype=torch.float32, device=self.device)
        for _ in range(self.niter):
            a = self.assign_device(x, c)
            order, list_off, counts = self._group(a)
            _lib.check(lib.wise_ivf_list_sums(x.data_ptr(), order.data_ptr(), list_off.data_ptr(), self.nlist, self.d,
                                              sums.data_ptr(), st), "wise_ivf_list_sums")
            self._reseed_empty(sums, counts)
            _lib.check(lib.wise_ivf_normalize_rows(sums.data_ptr(), self.nlist, self.d, c.data_ptr(), st),
                       "wise_ivf_normalize_rows")    # spherical: unit centroids
        self._install(c)

    def _seed_rows(self, x: torch.Tensor) -> torch.Tensor:
        """[nlist, d]: the rows of x at randperm(n, seed)[:nlist], the initial centroids of either k-means, as they are"""
        g = torch.Generator(device="cpu").manual_seed(self.seed)
        perm = torch.randperm(x.shape[0], generator=g)[: self.nlist].to(self.device)
        return self._gather_rows(x, perm)

    def _reseed_empty(self, cells: torch.Tensor, counts: torch.Tensor) -> None:
        """The host decision on empty cells and wise_ivf_reseed: every row of `cells` [nlist, d] (the sums, or the means of the plain
        k-means) whose cell is empty becomes a slightly perturbed copy of a fullest cell's row (ties: the lower cell first)."""
        cnt = counts.cpu().numpy()                           # nlist numbers: which cells are empty is decided on the host
        empty = np.flatnonzero(cnt == 0)
        if empty.size:
            donors = np.argsort(-cnt, kind="stable")[: empty.size]
            e_d = torch.from_numpy(empty.astype(np.int64)).to(self.device)
            d_d = torch.from_numpy(donors.astype(np.int64)).to(self.device)
            _lib.check(_lib.lib().wise_ivf_reseed(cells.data_ptr(), e_d.data_ptr(), d_d.data_ptr(), int(empty.size), self.d,
                                                  _lib.stream_ptr()), "wise_ivf_reseed")

    def set_centroids(self, centroids) -> None:
        """Install a trained quantizer (file load, tests)."""
        c = _as_tensor(centroids, np.float32)
        if c.shape != (self.nlist, self.d):
            raise ValueError(f"set_centroids: expected [{self.nlist},{self.d}]")
        self._install(c.to(self.device, torch.float32))

    def _install(self, c: torch.Tensor) -> None:
        self.centroids = c.contiguous()
        self._quantizer = FlatIPIndex(self.d, device=str(self.device)).adopt(self.centroids, None, id_base=0)
        self.is_trained = True

    def probes_device(self, q: torch.Tensor, nprobe: int) -> torch.Tensor:
        """[nq, nprobe] int64 list numbers: the nprobe centroids of largest inner product (-1 padding when
        nprobe > nlist).  Few probes: the flat top-k kernel over the centroid table.  Many probes (threshold lists
        stop filtering when k is a sizeable fraction of nlist): all centroid scores in exact fp32 on the matrix
        cores (wise_ip_scores_f32), then the radix-select kernel; the probes then come in list order, which the
        list scan does not care about."""
        if nprobe <= 64:
            _, I = self._quantizer.search_device(q, nprobe)
            return I
        lib = _lib.lib()
        scores = torch.empty(q.shape[0], self.nlist, dtype=torch.float32, device=self.device)
        rc = lib.wise_ip_scores_f32(self.centroids.data_ptr(), self.nlist, self.d, q.data_ptr(), q.shape[0],
                                    scores.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "wise_ip_scores_f32")
        out = torch.empty(q.shape[0], nprobe, dtype=torch.int64, device=self.device)
        rc = lib.wise_select_topk_f32(scores.data_ptr(), q.shape[0], self.nlist, nprobe, out.data_ptr(),
                                      _lib.stream_ptr())
        _lib.check(rc, "wise_select_topk_f32")
        return out


class L2CoarseQuantizer(CoarseQuantizer):
    """The coarse stage of IndexIVFFlatL2 (ivf_flat.py: IVFFlatL2Index): the nearest centroid under squared L2, and a plain
    (non-spherical) k-means.  THE COARSE RULE (include/wise_hip.h): g(x, c) = fl(s(x, c) - h_c), s wise_ip_scores_f32's chain and
    h_c = |c|^2 / 2 (wise_l2_half_norms); a row goes to argmax_c g (ties: the lowest c), a query probes the nprobe largest g —
    ONE path for every nprobe, so assignment and probing share their arithmetic and a stored row's own list is among its probes
    at any nprobe >= 1.  Grouping, gathering, seeding and the decision on empty cells are CoarseQuantizer's."""

    def __init__(self, d: int, nlist: int, device: str = "cuda"):
        super().__init__(d, nlist, device)
        self.half: Optional[torch.Tensor] = None         # [nlist] fp32: h_c of the installed centroids

    @staticmethod
    def half_norms(c: torch.Tensor) -> torch.Tensor:
        half = torch.empty(c.shape[0], dtype=torch.float32, device=c.device)
        _lib.check(_lib.lib().wise_l2_half_norms(c.data_ptr(), c.shape[0], c.shape[1], half.data_ptr(), _lib.stream_ptr()),
                   "wise_l2_half_norms")
        return half

    @staticmethod
    def scores_device(q: torch.Tensor, c: torch.Tensor, half: torch.Tensor, scores: torch.Tensor) -> None:
        """scores[:nq] = g(q, c) for every (row of q, centroid)"""
        lib, st = _lib.lib(), _lib.stream_ptr()
        _lib.check(lib.wise_ip_scores_f32(c.data_ptr(), c.shape[0], c.shape[1], q.data_ptr(), q.shape[0], scores.data_ptr(), st),
                   "wise_ip_scores_f32")
        _lib.check(lib.wise_ivf_l2_coarse(scores.data_ptr(), half.data_ptr(), q.shape[0], c.shape[0], st), "wise_ivf_l2_coarse")

    def assign_device(self, x: torch.Tensor, centroids: torch.Tensor, chunk: int = 4096, half: Optional[torch.Tensor] = None) -> torch.Tensor:
        """nearest centroid of every row by the coarse rule; half: h_c of `centroids` when the caller has it (the installed ones':
        looked up here)"""
        lib = _lib.lib()
        c = centroids.contiguous()
        if half is None:
            half = self.half if centroids is self.centroids else self.half_norms(c)
        out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
        scores = torch.empty(min(chunk, max(x.shape[0], 1)), c.shape[0], dtype=torch.float32, device=x.device)
        for s in range(0, x.shape[0], chunk):
            q = x[s:s + chunk]
            self.scores_device(q, c, half, scores)
            _lib.check(lib.wise_ivf_argmax(scores.data_ptr(), q.shape[0], c.shape[0], out[s:].data_ptr(), _lib.stream_ptr()),
                       "wise_ivf_argmax")
        return out

    def train(self, x) -> None:
        """Plain k-means, deterministic: the seeds are rows of x as they are; `niter` times the coarse rule, wise_ivf_group,
        wise_ivf_list_sums, wise_ivf_list_means (an empty cell keeps its sum, zeros), then on the means the decision on empty cells
        and wise_ivf_reseed."""
        lib = _lib.lib()
        x = _as_tensor(x, np.float32).to(self.device, torch.float32).contiguous()
        _rows_f32(x, self.d, "train")
        if x.shape[0] < self.nlist:
            raise ValueError(f"train: {x.shape[0]} training vectors for {self.nlist} cells")
        st = _lib.stream_ptr()
        c = self._seed_rows(x)
        for _ in range(self.niter):
            a = self.assign_device(x, c, half=self.half_norms(c))
            order, list_off, counts = self._group(a)
            _lib.check(lib.wise_ivf_list_sums(x.data_ptr(), order.data_ptr(), list_off.data_ptr(), self.nlist, self.d, c.data_ptr(), st),
                       "wise_ivf_list_sums")
            _lib.check(lib.wise_ivf_list_means(c.data_ptr(), counts.data_ptr(), self.nlist, self.d, c.data_ptr(), st), "wise_ivf_list_means")
            self._reseed_empty(c, counts)
        self._install(c)

    def _install(self, c: torch.Tensor) -> None:
        self.centroids = c.contiguous()
        self.half = self.half_norms(self.centroids)
        self.is_trained = True

    def probes_device(self, q: torch.Tensor, nprobe: int) -> torch.Tensor:
        """[nq, nprobe] int64 list numbers in list order: the nprobe centroids of largest g (-1 padding when nprobe > nlist)"""
        scores = torch.empty(q.shape[0], self.nlist, dtype=torch.float32, device=self.device)
        self.scores_device(q, self.centroids, self.half, scores)
        out = torch.empty(q.shape[0], nprobe, dtype=torch.int64, device=self.device)
        _lib.check(_lib.lib().wise_select_topk_f32(scores.data_ptr(), q.shape[0], self.nlist, nprobe, out.data_ptr(), _lib.stream_ptr()),
                   "wise_select_topk_f32")
        return out


class ListStore:
    """`data` [N, width] (fp32 rows or uint8 codes) and `ids` [N] grouped by list, `list_off` [nlist + 1] int64; `n` counts
    the chunks not yet merged too.  Contract: within a list, rows stay in their order of insertion (the grouping is a stable
    sort and the rows already stored come first) — the sharded index's bit-equality with the one-GPU index rests on it.
    `gather(data, order)` is the per-dtype row gather (wise_ivf_gather_rows / wise_pq_gather_codes).
    `extra_gathers`: one gather per further per-row array; `extra` then holds those arrays ([N, ...], first dimension = row),
    passed to `append` / `adopt` in that order, merged under the same stable order as the payload and counted by nbytes()."""

    def __init__(self, nlist: int, width: int, dtype: torch.dtype, device: torch.device, gather: Callable,
                 extra_gathers: Sequence[Callable] = ()):
        self.nlist, self.width, self.dtype, self.device, self._gather = nlist, width, dtype, device, gather
        self._extra_gathers = tuple(extra_gathers)
        self._pending: List[tuple] = []                  # (payload, ids, assign, extra) chunks not yet merged into the lists
        self.extra: List[torch.Tensor] = []
        self.data: Optional[torch.Tensor] = None
        self.ids: Optional[torch.Tensor] = None
        self.list_off: Optional[torch.Tensor] = None
        self.n = 0
        self.version = 0                                 # counts what changed the rows (append, adopt, compact): group tables belong to one value

    def _check_extra(self, extra: Sequence[torch.Tensor], n: int) -> tuple:
        if len(extra) != len(self._extra_gathers) or any(t.shape[0] != n for t in extra):
            raise ValueError(f"ListStore: expected {len(self._extra_gathers)} extra arrays of {n} rows")
        return tuple(extra)

    def append(self, payload: torch.Tensor, ids: torch.Tensor, assign: torch.Tensor, extra: Sequence[torch.Tensor] = ()) -> None:
        self._pending.append((payload, ids, assign, self._check_extra(extra, payload.shape[0])))
        self.n += payload.shape[0]
        self.version += 1

    def adopt(self, data: torch.Tensor, ids: torch.Tensor, list_off: torch.Tensor, extra: Sequence[torch.Tensor] = ()) -> None:
        """Take a payload that is already grouped by list (file load); chunks not yet merged are dropped."""
        self._pending = []
        self.extra = [t.to(self.device).contiguous() for t in self._check_extra(extra, data.shape[0])]
        self.data = data.to(self.device, self.dtype).contiguous()
        self.ids = ids.to(self.device, torch.int64).contiguous()
        self.list_off = list_off.to(self.device, torch.int64).contiguous()
        self.n = self.data.shape[0]
        self.version += 1

    def finalize(self, group: Callable) -> None:
        """Merge the pending chunks into the lists; `group` is the quantizer's stable grouping (CoarseQuantizer._group)."""
        if self._pending:
            lib = _lib.lib()
            st = _lib.stream_ptr()
            old = [(self.data, self.ids, None, tuple(self.extra))] if self.data is not None and self.data.shape[0] else []
            old_assign = []
            if old:
                oa = torch.empty(self.data.shape[0], dtype=torch.int64, device=self.device)     # the rows already grouped: list c, list_off[c] .. [c + 1]
                _lib.check(lib.wise_ivf_expand_lists(self.list_off.data_ptr(), self.nlist, oa.data_ptr(), st), "wise_ivf_expand_lists")
                old_assign = [oa]
            a = torch.cat(old_assign + [p[2] for p in self._pending]).contiguous()
            order, list_off, _ = group(a)
            alld = torch.cat([p[0] for p in old + self._pending]).contiguous()
            allids = torch.cat([p[1] for p in old + self._pending]).contiguous()
            self.data = self._gather(alld, order)
            self.extra = [g(torch.cat([p[3][e] for p in old + self._pending]).contiguous(), order)
                          for e, g in enumerate(self._extra_gathers)]
            ids = torch.empty_like(allids)
            _lib.check(lib.wise_ivf_gather_i64(allids.data_ptr(), order.data_ptr(), order.shape[0], ids.data_ptr(), st), "wise_ivf_gather_i64")
            self.ids, self.list_off, self._pending = ids, list_off, []
        if self.data is None:
            self.data = torch.empty(0, self.width, dtype=self.dtype, device=self.device)
            self.ids = torch.empty(0, dtype=torch.int64, device=self.device)
            self.list_off = torch.zeros(self.nlist + 1, dtype=torch.int64, device=self.device)

    def compact(self, c) -> None:
        """remove_ids on the merged lists (no pending chunks): every per-row array compacted in place under the one plan of
        `c` (mutate.RowCompaction) and narrowed to the kept rows — views of the same allocations, nothing is copied or given
        back —, list_off re-ranked.  Within a list the rows keep their order."""
        if self._pending or self.data is None or self.data.shape[0] != c.n:
            raise RuntimeError("ListStore.compact: merge the pending chunks first")
        self.list_off = c.rank(self.list_off)
        self.data, self.ids = c.rows(self.data), c.rows(self.ids)
        self.extra = [c.rows(t) for t in self.extra]
        self.n = c.kept
        self.version += 1

    def nbytes(self) -> int:
        """Bytes of HBM the merged lists hold: payload, ids, offsets, extra arrays."""
        return sum(t.numel() * t.element_size() for t in (self.data, self.ids, self.list_off, *self.extra))


class IVFIndexBase(_group.GroupTables):
    """One CoarseQuantizer (`_coarse`), one ListStore (`_lists`), and the surface both indexes show around them."""

    COARSE = CoarseQuantizer      # the class of `_coarse` (IVFFlatL2Index: L2CoarseQuantizer)
    metric = "ip"                 # 'l2': distances, ascending (IVFFlatL2Index); the sharded wrappers and range_search read it
    GROUP_SCORES: Optional[str] = None   # stage 1 of search_grouped in the C ABI; None: the type has none (product-quantized)

    def __init__(self, d: int, nlist: int, device: str, width: int, dtype: torch.dtype, gather: Callable,
                 extra_gathers: Sequence[Callable] = ()):
        self._coarse = self.COARSE(d, nlist, device)
        self.d, self.nlist, self.device = self._coarse.d, self._coarse.nlist, self._coarse.device
        self._lists = ListStore(self.nlist, width, dtype, self.device, gather, extra_gathers)
        self.nprobe = 1           # faiss default; the REST layer sets it (routes.py:902)
        self.parallel_mode = 0    # accepted and ignored (routes.py:901)
        self.direct_map = _DirectMap()
        self._ws: Optional[torch.Tensor] = None

    @property
    def ntotal(self) -> int:
        return self._lists.n

    @property
    def centroids(self) -> Optional[torch.Tensor]:
        return self._coarse.centroids

    @property
    def is_trained(self) -> bool:
        return self._coarse.is_trained

    def set_centroids(self, centroids) -> None:
        self._coarse.set_centroids(centroids)

    def probes_device(self, q: torch.Tensor, nprobe: int) -> torch.Tensor:
        return self._coarse.probes_device(q, nprobe)

    def _finalize(self) -> None:
        self._lists.finalize(self._coarse._group)

    def _queries(self, q: torch.Tensor) -> torch.Tensor:
        """The start of every search: the lists merged, q [nq,d] checked and on the device as contiguous fp32."""
        if not self.is_trained:
            raise RuntimeError(f"{type(self).__name__}: not trained")
        self._finalize()
        if q.dim() != 2 or q.shape[1] != self.d:
            raise ValueError(f"search: expected [nq,{self.d}], got {tuple(q.shape)}")
        return q.to(self.device, torch.float32).contiguous()

    def _selector_rows(self):
        """(external ids in list order on the device, id_base = 0, row count) of the merged lists: what a selector is resolved
        against."""
        self._finalize()
        return self._lists.ids, 0, self._lists.n

    def _keep(self, sel) -> Optional[torch.Tensor]:
        """The bitmap over list positions a scan tests (selector.py), None without a selector."""
        res = resolve_for(self, sel)
        return None if res is None else res.bitmap

    def _clamped_nprobe(self) -> int:
        return max(1, min(int(self.nprobe), self.nlist, 2048))

    def _workspace(self, need: int) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def search(self, x, k: int, params=None):
        """faiss signature: x np.ndarray [nq,d] float32 -> (D, I) numpy.
        params: SearchParametersIVF(sel=..., nprobe=...) — the coarse stage probes the same lists, only the selected rows
        compete; nprobe replaces the index's for this call only."""
        sel, nprobe = unpack_params(params, ivf=True)
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2:
            raise ValueError("search: x must be 2-D")
        q = torch.from_numpy(x).to(self.device)
        kept = self.nprobe
        try:
            if nprobe is not None:
                self.nprobe = nprobe
            D, I = self.search_device(q, int(k)) if sel is None else self.search_device(q, int(k), sel=sel)
        finally:
            self.nprobe = kept
        return D.cpu().numpy(), I.cpu().numpy()

    # -- range search: the part every inverted-file type shares (range_search.py) ----------------
    def _range_workspace_bytes(self, nq: int, nprobe: int) -> int:
        """The type's *_range_workspace_bytes; the types without a range search (product-quantized) do not override it."""
        raise NotImplementedError(_range.UNSUPPORTED.format(type(self).__name__))

    def _range_stage(self, qs: torch.Tensor, probes: torch.Tensor, nprobe: int, radius: float, keep: Optional[torch.Tensor]):
        """(count, fill) of range_search.run for the queries qs and their probes: the type's count / fill pair of the C ABI."""
        raise NotImplementedError(_range.UNSUPPORTED.format(type(self).__name__))

    def range_search_device(self, q: torch.Tensor, thresh: float, sel=None, chunk: Optional[int] = None):
        """q [nq,d] fp32 on device -> (lims [nq+1] int64, D fp32, I int64) on the device: every row OF THE PROBED LISTS with
        score > thresh (faiss's IVF range search), each query's segment by descending score, ties by ascending list position.
        sel: only the selected rows can be hits.  chunk: queries per workspace chunk."""
        self._range_workspace_bytes(1, 1)                # NotImplementedError on the types without a range search
        radius = _range.check_threshold(thresh)
        q = self._queries(q)
        keep = self._keep(sel)
        nprobe = self._clamped_nprobe()

        def stage(qs):
            return self._range_stage(qs, self._coarse.probes_device(qs, nprobe).contiguous(), nprobe, radius, keep)

        return _range.run(q, lambda m: self._range_workspace_bytes(m, nprobe), stage, self._workspace, self._lists.ids, 0, chunk,
                          ascending=self.metric == "l2")

    def range_search(self, x, thresh: float, params=None):
        """faiss signature: x np.ndarray [nq,d] float32 -> (lims, D, I) numpy.  params: SearchParametersIVF(sel=..., nprobe=...);
        nprobe replaces the index's for this call only."""
        self._range_workspace_bytes(1, 1)
        sel, nprobe = unpack_params(params, ivf=True)
        q = _range.to_numpy(x).to(self.device)
        kept = self.nprobe
        try:
            if nprobe is not None:
                self.nprobe = nprobe
            lims, D, I = self.range_search_device(q, thresh, sel=sel)
        finally:
            self.nprobe = kept
        return lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()

    # -- grouped search: the part every inverted-file type shares (group_search.py: set_groups, clear_groups, ngroups, search_grouped)
    def _rows_version(self) -> int:
        return self._lists.version

    def _group_refusal(self) -> None:
        if self.GROUP_SCORES is None:
            raise NotImplementedError(_group.UNSUPPORTED.format(type(self).__name__))
        if getattr(self, "pos_base", 0) != 0:
            raise NotImplementedError(_group.NO_SLICE.format(type(self).__name__, self.pos_base))

    def _group_scores(self, lib, st: int, qs: torch.Tensor, probes: torch.Tensor, nprobe: int, keep: Optional[torch.Tensor], ord_ptr: int) -> None:
        """The type's GROUP_SCORES call for the queries qs and their probes: the lists' fp32 rows take the queries as they are"""
        ls = self._lists
        _lib.check(getattr(lib, self.GROUP_SCORES)(ls.data.data_ptr(), ls.n, self.d, ls.list_off.data_ptr(), self.nlist, qs.data_ptr(),
                                                   qs.shape[0], probes.data_ptr(), nprobe, _lib.ptr(keep), ord_ptr, st), self.GROUP_SCORES)

    def search_grouped_device(self, q: torch.Tensor, k: int, sel=None, chunk: Optional[int] = None):
        """q [nq,d] fp32 on device -> (D [nq,k] fp32, I [nq,k] int64, G [nq,k] int64) on the device, no host sync: the k best
        groups among the rows OF THE PROBED LISTS, each with its best row (group_search.py); nprobe and the coarse rule are
        search's.  sel: only the selected rows are candidates.  chunk: queries per workspace chunk.  RuntimeError before set_groups."""
        tables = self._need_groups()
        lib = _lib.lib()
        q = self._queries(q)
        keep = self._keep(sel)
        nprobe, st = self._clamped_nprobe(), _lib.stream_ptr()

        def scores(qs, ord_ptr):
            self._group_scores(lib, st, qs, self._coarse.probes_device(qs, nprobe).contiguous(), nprobe, keep, ord_ptr)

        return _group.run(q, k, tables, scores, self._workspace, self._lists.ids, 0, self.metric, chunk)

    REMOVE_SCRATCH_BYTES = _mutate.SCRATCH_BYTES

    def remove_ids(self, sel, scratch_bytes: Optional[int] = None) -> int:
        """faiss's Index::remove_ids: drop the rows `sel` selects (an IDSelector, or an array of ids); returns how many went.
        Afterwards the index is, byte for byte, the one with the same trained state that was given only the kept rows in the
        same order.  Pending rows are merged first; the arrays are compacted in place (csrc/compact.hip) through a scratch of
        `scratch_bytes` (default REMOVE_SCRATCH_BYTES), so the extra memory does not grow with the index.  The direct map is a
        lookup in the stored id array, which is compacted too: a removed id reconstructs to NaN."""
        if getattr(self, "pos_base", 0) != 0:
            raise NotImplementedError(f"{type(self).__name__}.remove_ids: this index is a slice of a sharded index "
                                      f"(pos_base = {self.pos_base}); a collective removal is not built")
        c = _mutate.start(self, sel, scratch_bytes)      # resolves against the merged lists (_selector_rows finalizes)
        if c is None:
            return 0
        self._lists.compact(c)
        self._mutations = getattr(self, "_mutations", 0) + 1
        return c.n - c.kept

    def make_direct_map(self, enable: bool = True) -> None:
        """routes.py:904-909: afterwards reconstruct works by id.  Ids are looked up in the stored id array."""
        self.direct_map.type = _DirectMap.Hashtable if enable else _DirectMap.NoMap


class CodedIVFIndexBase(IVFIndexBase):
    """An inverted-file index whose lists hold ENCODED RESIDUALS (ivf_sq.py, ivf_pq.py): building the lists, the one-stage
    search with its selector and rank-local forms, and the id lookup, once.  Across GPUs an index holds one rank's slice of
    the list-major arrays: list_off clipped to the slice and `pos_base`, the position of its first row in the whole array.
    A codec supplies its scan entry points and workspace functions by name (below) and
      _payload(xs, assign)   the encoded rows of a chunk (what the lists keep of it)
      _operands(lib, st, qs) the per-query tensors its scan takes between `ids` and `nq`
    and, where it has them, _extra_rows / _adopted_extra (further per-row arrays), `_workspace_extra` with `_shape_suffix`
    (further arguments of its workspace functions) and WHO (a fixed class name for its error texts).
    `lib` and `st` are the handle and the stream the caller has from _lib.lib() and _lib.stream_ptr(): a search of one query
    is a handful of launches, and the device and the stream are asked for once per scan, not once per helper."""
    SCAN = SCAN_SEL = SCAN_LOCAL = WORKSPACE = WORKSPACE_LOCAL = None       # names of the C ABI
    WHO: Optional[str] = None                                                # None: the class's own name

    def __init__(self, d: int, nlist: int, device: str, width: int, dtype: torch.dtype, gather: Callable,
                 extra_gathers: Sequence[Callable] = ()):
        super().__init__(d, nlist, device, width, dtype, gather, extra_gathers)
        self.pos_base = 0         # position of the first row in the whole list-major array (a rank's slice: adopt_lists)
        self._workspace_extra: tuple = ()                # what the workspace functions take after (nq, nprobe, k) ...
        self._shape_suffix = ""                          # ... and how an "unsupported shape" text names it

    def _payload(self, xs: torch.Tensor, assign: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def _operands(self, lib, st: int, qs: torch.Tensor) -> tuple:
        raise NotImplementedError

    def _extra_rows(self, xs: torch.Tensor) -> tuple:
        """What else the lists keep of a chunk of rows (nothing: the codes are all there is)."""
        return ()

    def _adopted_extra(self, n: int, *extra) -> tuple:
        """adopt_lists: the further per-row arrays of n adopted rows, checked (none here)."""
        return ()

    def _residuals(self, x: torch.Tensor, assign: torch.Tensor) -> torch.Tensor:
        out = torch.empty_like(x)
        _lib.check(_lib.lib().wise_pq_residuals(x.data_ptr(), self.centroids.data_ptr(), assign.data_ptr(), x.shape[0], self.d,
                                                self.nlist, out.data_ptr(), _lib.stream_ptr()), "wise_pq_residuals")
        return out

    def _bias(self, lib, st: int, qs: torch.Tensor, probes: torch.Tensor, nprobe: int) -> torch.Tensor:
        """[n, nprobe] fp32: q . c_l for every probe of every query."""
        bias = torch.empty(qs.shape[0], nprobe, dtype=torch.float32, device=self.device)
        _lib.check(lib.wise_pq_bias(qs.data_ptr(), self.centroids.data_ptr(), probes.data_ptr(), qs.shape[0], nprobe, self.nlist,
                                    self.d, bias.data_ptr(), st), "wise_pq_bias")
        return bias

    # -- construction ---------------------------------------------------------------------------
    def _encoded_chunks(self, x: torch.Tensor, chunk: int):
        """(start, assign, payload, extra rows) per chunk: the fp32 rows live on the device one chunk at a time, never longer"""
        for s in range(0, x.shape[0], chunk):
            xs = x[s:s + chunk].to(self.device, torch.float32).contiguous()
            a = self._coarse.assign_device(xs, self.centroids)
            yield s, a, self._payload(xs, a), self._extra_rows(xs)

    def add_with_ids(self, x, ids, chunk: int = 1 << 18) -> None:
        if not self.is_trained:
            raise RuntimeError(f"{self.WHO or type(self).__name__}: train() before add_with_ids()")
        x = _rows_f32(x, self.d, "add_with_ids")
        ids = _ids_i64(ids, x.shape[0])
        for s, a, payload, extra in self._encoded_chunks(x, chunk):
            self._lists.append(payload, ids[s:s + chunk].to(self.device, torch.int64).contiguous(), a, extra)

    def encode_rows(self, x, chunk: int = 1 << 18):
        """(assign [n] int64, payload [n, width], extra per-row arrays ...) as numpy for the rows x [n, d]: what add_with_ids
        would put into the lists, handed back instead (the collective build moves it to the rank that owns the row's position)."""
        if not self.is_trained:
            raise RuntimeError(f"{self.WHO or type(self).__name__}: train() before encode_rows()")
        x = _rows_f32(x, self.d, "encode_rows")
        out = None
        for s, *parts in self._encoded_chunks(x, chunk):
            parts = [t.cpu().numpy() for t in (parts[0], parts[1], *parts[2])]
            if out is None:
                out = [np.empty((x.shape[0],) + t.shape[1:], dtype=t.dtype) for t in parts]
            for o, t in zip(out, parts):
                o[s:s + t.shape[0]] = t
        if out is None:
            ls = self._lists
            xs = torch.empty(0, self.d, dtype=torch.float32, device=self.device)
            out = [np.empty(0, np.int64), torch.empty(0, ls.width, dtype=ls.dtype).numpy()] + [t.cpu().numpy() for t in self._extra_rows(xs)]
        return tuple(out)

    def adopt_lists(self, codes: torch.Tensor, ids: torch.Tensor, list_off: torch.Tensor, pos_base: int = 0,
                    extra: Sequence[torch.Tensor] = ()):
        """Take codes that are already grouped by list (file load).  pos_base: the codes are a slice of a larger list-major
        array that starts at this position of it (list_off clipped to the slice).  extra: what the class's _adopted_extra
        takes, checked after the codes and pos_base."""
        if codes.dim() != 2 or codes.shape[1] != self._lists.width:
            raise ValueError(f"adopt_lists: expected codes [n,{self._lists.width}]")
        if pos_base < 0:
            raise ValueError("adopt_lists: pos_base must not be negative")
        self._lists.adopt(codes, ids, list_off, self._adopted_extra(codes.shape[0], *extra))
        self.pos_base = int(pos_base)
        return self

    # -- search ---------------------------------------------------------------------------------
    def _scan(self, qs: torch.Tensor, k: int, D: torch.Tensor, I: torch.Tensor, positions: bool = False, local: bool = False,
              probe_count: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None) -> None:
        """Coarse stage, bias, the codec's operands and its scan for the queries qs into D / I [n, k]; positions: I receives
        positions in the lists instead of external ids.  local: SCAN_LOCAL — the probes whose list is empty in this slice are
        dropped first (the number kept goes to probe_count when given) and positions are those of the WHOLE array.
        keep: a selector's bitmap over the list positions (IVFIndexBase._keep) — SCAN_SEL, only those rows compete."""
        lib = _lib.lib()
        nprobe, ls, st, n = self._clamped_nprobe(), self._lists, _lib.stream_ptr(), qs.shape[0]
        need = getattr(lib, self.WORKSPACE_LOCAL if local else self.WORKSPACE)(n, nprobe, k, *self._workspace_extra)
        if need == 0:
            raise ValueError(f"search: unsupported shape nq={n} nprobe={nprobe} k={k}{self._shape_suffix}")
        ws = self._workspace(need)
        probes = self._coarse.probes_device(qs, nprobe).contiguous()
        bias = self._bias(lib, st, qs, probes, nprobe)
        operands = self._operands(lib, st, qs)
        head = (ls.data.data_ptr(), ls.n, ls.width, ls.list_off.data_ptr(), self.nlist, 0 if positions else ls.ids.data_ptr(),
                *[t.data_ptr() for t in operands], n, probes.data_ptr(), bias.data_ptr(), nprobe, k)
        tail = (ws.data_ptr(), ws.numel(), st)
        if local:
            _lib.check(getattr(lib, self.SCAN_LOCAL)(*head, self.pos_base, D.data_ptr(), I.data_ptr(), _lib.ptr(probe_count), *tail),
                       self.SCAN_LOCAL)
        elif keep is not None:
            _lib.check(getattr(lib, self.SCAN_SEL)(*head, keep.data_ptr(), D.data_ptr(), I.data_ptr(), *tail), self.SCAN_SEL)
        else:
            _lib.check(getattr(lib, self.SCAN)(*head, D.data_ptr(), I.data_ptr(), *tail), self.SCAN)

    def _search(self, q: torch.Tensor, k: int, chunk: int, positions: bool = False, local: bool = False,
                probe_count: Optional[torch.Tensor] = None, sel=None):
        q = self._queries(q)
        keep = self._keep(sel)
        nq = q.shape[0]
        if probe_count is not None and (probe_count.dtype != torch.int32 or probe_count.numel() < nq or probe_count.device != q.device
                                        or not probe_count.is_contiguous()):
            raise ValueError("search_local_device: probe_count must be a contiguous int32 device tensor of nq entries")
        D = torch.empty(nq, k, dtype=torch.float32, device=self.device)
        I = torch.empty(nq, k, dtype=torch.int64, device=self.device)
        for s in range(0, nq, chunk):                    # bounds the workspace and the operands: chunk queries at a time
            self._scan(q[s:s + chunk], k, D[s:s + chunk], I[s:s + chunk], positions, local,
                       None if probe_count is None else probe_count[s:s + chunk], keep)
        return D, I

    def search_device(self, q: torch.Tensor, k: int, chunk: int = 1024, sel=None):
        """sel: an IDSelector (selector.py) — the same probes, only the selected rows compete."""
        return self._search(q, k, chunk, sel=sel)

    def search_local_device(self, q: torch.Tensor, k: int, probe_count: Optional[torch.Tensor] = None, positions: bool = False,
                            chunk: int = 1024):
        """search_device for an index that holds ONE RANK's slice of a list-major index sharded across GPUs (list_off clipped to
        the slice, `pos_base` its first position; sharded.py): the same coarse stage, bias and operands, then SCAN_LOCAL.
        probe_count: optional [nq] int32 device tensor that receives the number of probes kept per query.
        positions: I receives positions in the WHOLE array instead of external ids."""
        return self._search(q, k, chunk, positions, True, probe_count)

    def _positions(self, ids) -> torch.Tensor:
        """[n] int64 on the device: where each id sits in the lists (-1: unknown)."""
        self._finalize()
        ls = self._lists
        qi = torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int64)).to(self.device)
        pos = torch.empty(qi.numel(), dtype=torch.int64, device=self.device)
        _lib.check(_lib.lib().wise_pq_find(ls.ids.data_ptr(), ls.n, qi.data_ptr(), qi.numel(), pos.data_ptr(), _lib.stream_ptr()),
                   "wise_pq_find")
        return pos

"""faiss-shaped exhaustive inner-product indexes over 8-bit product-quantizer codes: IndexPQ<m> and its re-ranking forms
IndexPQ<m>R8 / IndexPQ<m>R16.

FlatPQIPIndex stands where `faiss.IndexIDMap(faiss.IndexPQ(d, m, 8, METRIC_INNER_PRODUCT))` would stand: the product quantizer of
IndexIVFPQ<m> (ivf_pq.py) without lists — no coarse k-means, no nprobe, no residuals; every row is scored.  HBM holds N (m + 8)
bytes of codes and ids and the codebooks [m, 256, d / m]; no fp32 rows.

  train(x)            the codebook trainer of IVFPQIPIndex (ivf_pq.py: PQCodebooks) on the rows themselves: rows perm[:65536] of a
                      seeded (1234) host permutation, the first 256 the initial codewords, 10 Lloyd iterations of wise_pq_encode /
                      wise_pq_update; deterministic
  add_with_ids(x,ids) the rows are encoded on the GPU chunk by chunk (wise_pq_encode) and only the codes are kept
  search(q, k)        one table per query (wise_pq_lut), then wise_pqflat_topk: score = +0 + sum_j lut[j][code_j], added in that order
                      in fp32 — bit for bit tests/pq_flat_ref.py; under a selector wise_pqflat_topk_pos over its positions
  reconstruct_batch   decoded, hence approximate, as in faiss: concat_j cb[j][code_j]; NaN for an unknown id
  range_search        not built, as on the inverted-file PQ types

FlatPQRefineIPIndex is the same index with faiss's IndexRefine around it: the rows are also kept, in row order, as compact rows —
int8 with a scale per row (d + 4 bytes, wise_ip_shadow_i8) or bf16 (2 d bytes, wise_ip_shadow_bf16) — and a search takes the
min(k * k_factor, 2048) best POSITIONS of the PQ scan and scores them again from those rows (wise_ivf_refine, the arithmetic of
tests/ivfpq_refine_ref.py).  reconstruct_batch returns the dequantised stored row.  PQ codes alone rank badly (tests/golden/
pq_flat_quality.json): the R forms are the useful ones.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from .. import _lib
from .flat_common import FlatIndexBase, RowStore
from .ivf_pq import DEFAULT_K_FACTOR, KSUB, MAX_CANDIDATES, MAX_TRAIN_ROWS, PQCodebooks, check_pq_shape, check_refine_shape
from .selector import resolve_for

PAD_SCORE = -3.4028234663852886e38


def _codes(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.uint8:
        raise ValueError(f"IndexPQ: uint8 codes expected, got {t.dtype}")
    return t


class FlatPQIPIndex(PQCodebooks, FlatIndexBase):
    ENCODE_BYTES = 64 << 20          # fp32 staging of add_with_ids: rows are encoded on the GPU this many bytes at a time
    QUERY_CHUNK = 1024               # queries whose tables (m KiB each) exist at once

    def __init__(self, d: int, m: int, device: str = "cuda"):
        check_pq_shape(int(d), int(m))
        super().__init__(d, device, torch.uint8, f"codes must be contiguous uint8 [N,{int(m)}] on the index's device")
        self.m, self.nbits, self.dsub = int(m), 8, int(d) // int(m)
        self._store = RowStore(self.m, torch.uint8, self.device, self._store.what)      # a row of the payload is m bytes, not d
        self.niter = 10
        self.seed = 1234
        self.codebooks: Optional[torch.Tensor] = None      # [m, 256, dsub] fp32
        self.is_trained = False

    # -- training -------------------------------------------------------------------------------
    def training_rows(self, x: torch.Tensor) -> torch.Tensor:
        """The rows the codebooks are trained on: rows perm[:65536] of x (seeded host permutation), in that order, on the device."""
        perm = np.random.default_rng(self.seed).permutation(x.shape[0])[:MAX_TRAIN_ROWS].astype(np.int64)
        idx = torch.from_numpy(perm)
        return x[idx.to(x.device)].to(self.device, torch.float32).contiguous()

    def train(self, x) -> None:
        """The codebooks from the rows x [n >= 256, d] (module docstring)."""
        x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        if x.dim() != 2 or x.shape[1] != self.d:
            raise ValueError(f"train: expected [n,{self.d}], got {tuple(x.shape)}")
        if x.shape[0] < KSUB:
            raise ValueError(f"train: {x.shape[0]} training vectors for {KSUB} codewords")
        if self._n:
            raise RuntimeError("IndexPQ: the index holds rows encoded against its codebooks; they cannot change")
        self.codebooks = self.train_codebooks(self.training_rows(x))
        self.is_trained = True

    def set_codebooks(self, codebooks) -> None:
        """Install trained codebooks [m, 256, dsub] (file load, tests).  Only an empty index is trained."""
        if self._n:
            raise RuntimeError("IndexPQ: the index holds rows encoded against its codebooks; they cannot change")
        super().set_codebooks(codebooks)
        self.is_trained = True

    def _need_trained(self, what: str) -> None:
        if not self.is_trained:
            raise RuntimeError(f"IndexPQ: {what} before train() or set_codebooks()")

    # -- construction ---------------------------------------------------------------------------
    @property
    def _codes_t(self) -> Optional[torch.Tensor]:
        """[N,m] uint8 on device: the whole payload"""
        return self._store.rows

    def hbm_bytes(self) -> int:
        """Bytes of HBM the index itself holds: the codes, the ids and the codebooks."""
        return self._n * (self.m + (8 if self._store.has_ids else 0)) + 4 * KSUB * self.d

    def add_with_ids(self, x, ids) -> None:
        self._need_trained("add_with_ids")
        super().add_with_ids(x, ids)

    def _fill(self, dst: torch.Tensor, x: torch.Tensor) -> None:
        """add_with_ids: the rows are encoded on the GPU (wise_pq_encode), chunk by chunk, so that no fp32 form of the index exists
        in HBM"""
        lib = _lib.lib()
        for s, part in self._staged(x):
            _lib.check(lib.wise_pq_encode(part.data_ptr(), self.codebooks.data_ptr(), part.shape[0], self.d, self.m,
                                          dst[s:s + part.shape[0]].data_ptr(), _lib.stream_ptr()), "wise_pq_encode")
            self._fill_extra(s, part)

    def _fill_extra(self, s: int, part: torch.Tensor) -> None:
        """what else a staged chunk of fp32 rows leaves behind (FlatPQRefineIPIndex: its compact rows)"""

    def add_codes_with_ids(self, codes, ids) -> None:
        """codes [n,m] uint8 (numpy or tensor), ids [n] int64: rows that are already encoded — an index file's — go to HBM as they
        are."""
        self._need_trained("add_codes_with_ids")
        c = _codes(codes if torch.is_tensor(codes) else torch.from_numpy(np.array(codes, dtype=np.uint8, order="C")))
        if c.dim() != 2 or c.shape[1] != self.m:
            raise ValueError(f"add_codes_with_ids: expected [n,{self.m}], got {tuple(c.shape)}")
        self._slot(c.shape[0], ids, "add_codes_with_ids").copy_(c)

    def adopt(self, codes: torch.Tensor, ids: Optional[torch.Tensor] = None, id_base: int = 0) -> "FlatPQIPIndex":
        """Take ownership of codes already resident in HBM (no copy).  ids None => id = id_base + row."""
        self._need_trained("adopt")
        return super().adopt(_codes(codes), ids, id_base)

    def _rows_changed(self) -> None:
        pass

    # -- search ---------------------------------------------------------------------------------
    def _tables(self, lib, qs: torch.Tensor, st: int) -> torch.Tensor:
        lut = torch.empty(qs.shape[0], self.m, KSUB, dtype=torch.float32, device=self.device)
        _lib.check(lib.wise_pq_lut(qs.data_ptr(), self.codebooks.data_ptr(), qs.shape[0], self.d, self.m, lut.data_ptr(), st), "wise_pq_lut")
        return lut

    def _scan(self, lib, qs: torch.Tensor, k: int, D: torch.Tensor, I: torch.Tensor, pos: Optional[torch.Tensor], positions: bool) -> None:
        """The PQ scan of the queries qs into D / I [n, k]: over every row, or over the rows pos[]; positions: I holds row
        positions (ids = NULL, id_base 0), what wise_ivf_refine takes."""
        st, n, nq = _lib.stream_ptr(), self._n, qs.shape[0]
        lut = self._tables(lib, qs, st)
        ids, id_base = (0, 0) if positions else (_lib.ptr(self._ids), self.id_base)
        items = n if pos is None else pos.numel()
        need = lib.wise_pqflat_topk_workspace_bytes(items, self.m, nq, k)
        if need == 0:
            raise ValueError(f"search: unsupported shape N={n} m={self.m} nq={nq} k={k}")
        ws = self._grown("_ws", need)
        C = _lib.ptr(self._codes_t)
        if pos is None:
            _lib.check(lib.wise_pqflat_topk(C, n, self.m, lut.data_ptr(), nq, k, ids, id_base, D.data_ptr(), I.data_ptr(), ws.data_ptr(),
                                            ws.numel(), st), "wise_pqflat_topk")
        else:
            _lib.check(lib.wise_pqflat_topk_pos(C, n, self.m, pos.data_ptr(), items, lut.data_ptr(), nq, k, ids, id_base, D.data_ptr(),
                                                I.data_ptr(), ws.data_ptr(), ws.numel(), st), "wise_pqflat_topk_pos")

    def _search_args(self, q: torch.Tensor, k: int, sel):
        self._need_trained("search")
        self._finalize()
        q = self._queries(q, "search")
        k = int(k)
        if k < 1 or k > MAX_CANDIDATES:
            raise ValueError(f"search: unsupported k={k} (1 <= k <= {MAX_CANDIDATES})")
        pos = None if sel is None else resolve_for(self, sel).positions()
        D = torch.empty(q.shape[0], k, dtype=torch.float32, device=self.device)
        I = torch.empty(q.shape[0], k, dtype=torch.int64, device=self.device)
        return q, k, pos, D, I

    def search_device(self, q: torch.Tensor, k: int, sel=None):
        """q [nq,d] fp32 on device -> (D [nq,k] fp32, I [nq,k] int64) on device, no host sync; capturable on one stream.
        sel: an IDSelector (selector.py) — only the rows it selects compete, by the scan over their positions."""
        lib = _lib.lib()
        q, k, pos, D, I = self._search_args(q, k, sel)
        for s in range(0, q.shape[0], self.QUERY_CHUNK):
            self._scan(lib, q[s:s + self.QUERY_CHUNK], k, D[s:s + self.QUERY_CHUNK], I[s:s + self.QUERY_CHUNK], pos, False)
        return D, I

    def range_search_device(self, q, thresh, sel=None, chunk=None):
        raise NotImplementedError("IndexPQ: range_search is not built on the product-quantizer types")

    def range_search(self, x, thresh, params=None):
        raise NotImplementedError("IndexPQ: range_search is not built on the product-quantizer types")

    def _group_refusal(self) -> None:
        from .group_search import UNSUPPORTED
        raise NotImplementedError(UNSUPPORTED.format("IndexPQ"))

    def search_grouped_device(self, q, k, sel=None, chunk=None):
        self._group_refusal()

    # -- the rest of the surface ------------------------------------------------------------------
    def _positions(self, ids) -> torch.Tensor:
        """[n] int64 on the device: the position of each external id (-1: not held)"""
        self._finalize()
        qi = torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int64)).reshape(-1).to(self.device)
        pos = torch.empty_like(qi)
        held = self._store.explicit_ids()
        _lib.check(_lib.lib().wise_pq_find(held.data_ptr(), self._n, qi.data_ptr(), qi.numel(), pos.data_ptr(), _lib.stream_ptr()),
                   "wise_pq_find")
        return pos

    def reconstruct_batch(self, ids) -> np.ndarray:
        """Decoded rows (approximate, as faiss's): the row's codewords side by side; NaN for an unknown id."""
        self._need_trained("reconstruct_batch")
        pos = self._positions(ids)
        out = torch.empty(pos.numel(), self.d, dtype=torch.float32, device=self.device)
        _lib.check(_lib.lib().wise_pqflat_decode(_lib.ptr(self._codes_t), self._n, pos.data_ptr(), pos.numel(), self.codebooks.data_ptr(),
                                                 self.d, self.m, out.data_ptr(), _lib.stream_ptr()), "wise_pqflat_decode")
        return out.cpu().numpy()

    def state_host(self) -> dict:
        """The index as the dict faiss_io.read_index returns for its file and faiss_io.write_index takes: codebooks [m,256,dsub],
        codes [N,m] uint8, ids [N]; the re-ranking class adds its store (rows of kind 16 as uint16 bit patterns)."""
        self._need_trained("state_host")
        codes, ids = self.rows_host()
        return dict(codebooks=self.codebooks.cpu().numpy(), codes=codes, ids=ids)


class FlatPQRefineIPIndex(FlatPQIPIndex):
    """FlatPQIPIndex + compact rows in row order + a re-ranking stage (module docstring).  `k_factor` as on faiss's IndexRefine: a
    search for k re-ranks the min(k * k_factor, 2048) best positions of the PQ scan."""

    def __init__(self, d: int, m: int, kind: int, k_factor: int = DEFAULT_K_FACTOR, device: str = "cuda"):
        check_refine_shape(int(d), int(kind))
        super().__init__(d, m, device)
        self.kind, self.k_factor = int(kind), int(k_factor)
        self._xrows: Optional[torch.Tensor] = None        # [N, d] int8, or int16 bf16 bit patterns: the merged compact rows
        self._xscales: Optional[torch.Tensor] = None      # [N] fp32 (kind 8)
        self._xrow_chunks: List[torch.Tensor] = []
        self._xscale_chunks: List[torch.Tensor] = []
        self._pending: Optional[tuple] = None             # the chunk add_with_ids is filling

    @property
    def _row_dtype(self) -> torch.dtype:
        return torch.int8 if self.kind == 8 else torch.int16          # int16: bf16 bit patterns

    def hbm_bytes(self) -> int:
        """the codes, ids and codebooks, and the compact rows (and scales)"""
        return super().hbm_bytes() + self._n * (self.d + 4 if self.kind == 8 else 2 * self.d)

    # -- construction ---------------------------------------------------------------------------
    # (reserve() holds room for the codes and ids; the compact rows are queued per add and merged once)
    def _fill(self, dst: torch.Tensor, x: torch.Tensor) -> None:
        n = x.shape[0]
        rows = torch.empty(n, self.d, dtype=self._row_dtype, device=self.device)
        scales = torch.empty(n, dtype=torch.float32, device=self.device) if self.kind == 8 else None
        self._pending = (rows, scales)
        super()._fill(dst, x)
        self._pending = None
        self._xrow_chunks.append(rows)
        if scales is not None:
            self._xscale_chunks.append(scales)

    def _fill_extra(self, s: int, part: torch.Tensor) -> None:
        lib, st = _lib.lib(), _lib.stream_ptr()
        rows, scales = self._pending
        n = part.shape[0]
        norms = torch.empty(4, dtype=torch.float32, device=self.device)      # the builders' error norms: scratch, not used here
        if self.kind == 8:
            _lib.check(lib.wise_ip_shadow_i8(part.data_ptr(), n, self.d, rows[s:s + n].data_ptr(), scales[s:s + n].data_ptr(),
                                             norms.data_ptr(), st), "wise_ip_shadow_i8")
        else:
            _lib.check(lib.wise_ip_shadow_bf16(part.data_ptr(), n, self.d, rows[s:s + n].data_ptr(), norms.data_ptr(), st),
                       "wise_ip_shadow_bf16")

    def add_codes_with_ids(self, codes, ids, rows=None, scales=None) -> None:
        """A file's rows as they are: codes [n,m] uint8, ids [n], compact rows [n,d] (int8; kind 16: int16 / uint16 bf16 bit patterns)
        and, for kind 8, scales [n] float32."""
        def as_t(v):
            if torch.is_tensor(v):
                return v
            v = np.array(v, order="C")
            return torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v)
        n = len(ids)
        if rows is None or (self.kind == 8 and scales is None):
            raise ValueError("add_codes_with_ids: the re-ranking index takes its compact rows (and scales) with the codes")
        r = as_t(rows)
        if tuple(r.shape) != (n, self.d) or r.dtype != self._row_dtype:
            raise ValueError(f"add_codes_with_ids: expected rows [{n},{self.d}] {self._row_dtype}")
        s = None
        if self.kind == 8:
            s = as_t(scales)
            if tuple(s.shape) != (n,) or s.dtype != torch.float32:
                raise ValueError(f"add_codes_with_ids: expected scales [{n}] float32")
        super().add_codes_with_ids(codes, ids)
        self._xrow_chunks.append(r.to(self.device).contiguous())
        if s is not None:
            self._xscale_chunks.append(s.to(self.device).contiguous())

    def adopt(self, codes, ids=None, id_base: int = 0):
        raise NotImplementedError("IndexPQ<m>R: adopt takes codes alone; use add_codes_with_ids with the compact rows")

    def _finalize(self) -> None:
        super()._finalize()
        if self._xrow_chunks or self._xrows is None:
            held = [self._xrows] if self._xrows is not None else []
            self._xrows = (torch.cat(held + self._xrow_chunks, dim=0).contiguous() if held or self._xrow_chunks
                           else torch.empty(0, self.d, dtype=self._row_dtype, device=self.device))
            self._xrow_chunks = []
        if self.kind == 8 and (self._xscale_chunks or self._xscales is None):
            held = [self._xscales] if self._xscales is not None else []
            self._xscales = (torch.cat(held + self._xscale_chunks, dim=0).contiguous() if held or self._xscale_chunks
                             else torch.empty(0, dtype=torch.float32, device=self.device))
            self._xscale_chunks = []

    def _compact_extra(self, c) -> None:
        """remove_ids: the compact rows and scales go through the plan the codes and ids went through"""
        self._xrows = c.rows(self._xrows)
        if self.kind == 8:
            self._xscales = c.rows(self._xscales)

    def _refine_store(self):
        """(rows pointer, scales pointer or 0) of the merged compact rows"""
        return self._xrows.data_ptr(), self._xscales.data_ptr() if self.kind == 8 else 0

    # -- search ---------------------------------------------------------------------------------
    def candidates(self, k: int) -> int:
        """How many positions of the PQ scan a search for k re-ranks."""
        return max(k, min(k * max(self.k_factor, 1), MAX_CANDIDATES))

    def search_device(self, q: torch.Tensor, k: int, sel=None):
        """sel: an IDSelector — the candidates are the k * k_factor best SELECTED rows of the PQ scan; the re-ranking is unchanged."""
        lib = _lib.lib()
        q, k, pos, D, I = self._search_args(q, k, sel)
        if self._n == 0:
            return D.fill_(PAD_SCORE), I.fill_(-1)
        kc, st = self.candidates(k), _lib.stream_ptr()
        rows, scales = self._refine_store()
        ids = self._store.explicit_ids()
        for s in range(0, q.shape[0], self.QUERY_CHUNK):
            qs = q[s:s + self.QUERY_CHUNK]
            n = qs.shape[0]
            cD = torch.empty(n, kc, dtype=torch.float32, device=self.device)
            cand = torch.empty(n, kc, dtype=torch.int64, device=self.device)
            self._scan(lib, qs, kc, cD, cand, pos, True)
            _lib.check(lib.wise_ivf_refine(rows, self.kind, scales, self._n, self.d, ids.data_ptr(), qs.data_ptr(), n, cand.data_ptr(), kc, k,
                                           D[s:s + n].data_ptr(), I[s:s + n].data_ptr(), st), "wise_ivf_refine")
        return D, I

    def reconstruct_batch(self, ids) -> np.ndarray:
        """The stored rows, dequantised (faiss's IndexRefine reconstructs from its refine index too); NaN for an unknown id."""
        pos = self._positions(ids)
        out = torch.empty(pos.numel(), self.d, dtype=torch.float32, device=self.device)
        if self._n == 0:
            return out.fill_(float("nan")).cpu().numpy()
        rows, scales = self._refine_store()
        _lib.check(_lib.lib().wise_ivf_refine_rows(rows, self.kind, scales, self._n, self.d, pos.data_ptr(), pos.numel(), out.data_ptr(),
                                                   _lib.stream_ptr()), "wise_ivf_refine_rows")
        return out.cpu().numpy()

    def store_host(self):
        """(rows [N,d] int8 or uint16 bf16 bits, scales [N] float32 or None) as numpy."""
        self._finalize()
        rows = self._xrows.cpu().numpy()
        return (rows, self._xscales.cpu().numpy()) if self.kind == 8 else (rows.view(np.uint16), None)

    def state_host(self) -> dict:
        rows, scales = self.store_host()
        return dict(super().state_host(), kind=self.kind, k_factor=self.k_factor, rows=rows, scales=scales)

"""search_grouped — "the k best GROUPS of rows (videos, shots, files), each with its best row" — for the index types whose scan
scores are exact functions of the stored rows: the exhaustive types (FlatIPIndex, FlatSQfp16IPIndex, FlatSQ8IPIndex, FlatL2Index,
FlatSQfp16L2Index) and the inverted-file types (IVFFlatIPIndex, IVFSQIPIndex, IVFSQfp16IPIndex, IVFFlatL2Index).

    index.set_groups(ids, keys)                       # keys[i] >= 0 is the group (e.g. the media id) of the stored id ids[i]
    D, I, G = index.search_grouped(x, k, params=None)

THE CONTRACT.  Every stored row carries a group key, an int64 >= 0.  For one query over its candidate rows — every row of an
exhaustive index, the rows of the probed lists of an inverted-file index (nprobe and the coarse rule as on `search`), under a
selector only the selected ones — a group's REPRESENTATIVE is its candidate row with the best score, ties to the lower row position
(the row of the payload; the position in list order for the inverted-file types): the tie rule of the scans.  The answer is the k
groups whose representatives are best, in the order of the representatives' (score, position) keys — descending score for the
inner-product types, ascending squared distance for the L2 types, which select on the negated distance like everything else.
D [nq, k] is the representative's score, bit for bit what the type's exact top-k scan gives that (query, row); I [nq, k] its
external id; G [nq, k] the group key.  Slots no group fills hold the type's padding score, -1 and -1; a group without a candidate
row does not appear.  The answer is not a prefix of anything `search` returns: grouping the top-k afterwards yields a dozen groups
when a thousand best frames come from a dozen files.

What this module holds is the part every type shares: the group tables (`build_group_tables`), their life on an index
(`GroupTables`), and the three stages of the C ABI (include/wise_hip.h, csrc/group_topk.hip) run over chunks of queries (`run`).
Stage 1 leaves 4 N bytes per query in the workspace and stage 2 another 8 G, so a batch is cut into chunks whose workspace stays
under range_search.WORKSPACE_BYTES (about 6 queries a chunk at 10M rows); there is no host round trip inside a chunk.
Groups are not written to index files — the formats are faiss's —, so a caller sets them after load_index.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
import torch

from .. import _lib
from . import range_search as _range
from .selector import unpack_params

UNSUPPORTED = ("{}: search_grouped is not implemented — the scores of the product-quantized types are approximate and a group's "
               "representative would depend on the re-ranking stage; the Flat, SQ and IVFFlat / IVFSQ types support it")
NO_SHARDED = ("search_grouped is not implemented on a sharded index: a group's rows may lie on several ranks and the exchange of "
              "per-group representatives is not built; the unsharded Flat, SQ and IVFFlat / IVFSQ types support it")
NO_SLICE = ("{}: search_grouped is not implemented on a slice of a sharded index (pos_base = {}): a group's rows may lie on "
            "several ranks")
NO_GROUPS = ("{}: search_grouped needs the rows' groups and the index holds none for its present rows (adding, removing or "
             "adopting rows drops them): call set_groups(ids, keys) first")


def build_group_tables(row_ids, id_base: int, n: int, ids, keys):
    """The group tables of n stored rows as numpy arrays: (gid [n] int32, group_keys [G] int64 ascending, group_off [G + 1] int64,
    group_rows [n] uint32 — the row positions sorted by (group, position)).
    row_ids: the stored external ids in row order ([n] int64), or None for the implicit ids id_base + row.
    ids, keys: keys[i] >= 0 is the group key of the external id ids[i].  Ids the index does not store are ignored; an id stored
    twice puts both rows into its group.  ValueError: ids and keys of different length, a negative key, one id given two
    different keys, a stored id that `ids` does not list (the first one in row order is named)."""
    ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
    keys = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)
    if ids.shape != keys.shape:
        raise ValueError(f"set_groups: ids and keys must have the same length, got {ids.size} and {keys.size}")
    if keys.size and int(keys.min()) < 0:
        raise ValueError(f"set_groups: a group key must not be negative, got {int(keys.min())}")
    n = int(n)
    if n >= 0xFFFFFFFF:
        raise ValueError(f"set_groups: {n} rows exceed the positions a key holds (2^32 - 1)")
    order = np.argsort(ids, kind="stable")
    sid, skey = ids[order], keys[order]
    clash = np.flatnonzero((sid[1:] == sid[:-1]) & (skey[1:] != skey[:-1]))
    if clash.size:
        i = int(clash[0])
        raise ValueError(f"set_groups: id {int(sid[i])} is given two different keys, {int(skey[i])} and {int(skey[i + 1])}")
    rows = (np.arange(n, dtype=np.int64) + int(id_base)) if row_ids is None else np.ascontiguousarray(row_ids, dtype=np.int64).reshape(-1)
    if rows.shape != (n,):
        raise ValueError(f"set_groups: {rows.size} stored ids for {n} rows")
    at = np.searchsorted(sid, rows)
    found = at < sid.size
    found[found] = sid[at[found]] == rows[found]
    if not bool(found.all()):
        raise ValueError(f"set_groups: the stored id {int(rows[int(np.argmin(found))])} has no group (it is not in ids)")
    group_keys, gid = np.unique(skey[at], return_inverse=True)
    if group_keys.size > 0x7FFFFFFF:
        raise ValueError(f"set_groups: {group_keys.size} groups exceed what gid holds (2^31 - 1)")
    gid = gid.reshape(-1)
    group_rows = np.argsort(gid, kind="stable")
    group_off = np.zeros(group_keys.size + 1, dtype=np.int64)
    np.cumsum(np.bincount(gid, minlength=group_keys.size), out=group_off[1:])
    return gid.astype(np.int32), group_keys.astype(np.int64), group_off, group_rows.astype(np.uint32)


class GroupTables:
    """The group tables of an index and the numpy surface of search_grouped, shared by FlatIndexBase and IVFIndexBase.  The tables
    live on the device beside the ids and belong to ONE state of the rows: the index reports that state through `_rows_version()`
    — a count of everything that changed its rows — and tables of another state are dropped where they are next looked at.
    A class gives `_selector_rows()` (ids, id_base, row count of the merged rows), `_rows_version()`, `search_grouped_device` and
    the `ivf` flag of its search parameters."""
    _groups: Optional[dict] = None

    def _group_refusal(self) -> None:
        """NotImplementedError where the type or this index has no search_grouped"""

    def set_groups(self, ids, keys) -> None:
        """keys[i] >= 0 is the group key (e.g. the media id) of the stored id ids[i] (build_group_tables: every stored id must be
        listed).  Holds until the rows change."""
        self._group_refusal()
        row_ids, id_base, n = self._selector_rows()
        gid, group_keys, group_off, group_rows = build_group_tables(None if row_ids is None else row_ids.cpu().numpy(), id_base, n, ids, keys)
        dev = self.device
        self._groups = dict(version=self._rows_version(), n=n, gid=torch.from_numpy(gid).to(dev), keys=torch.from_numpy(group_keys).to(dev),
                            off=torch.from_numpy(group_off).to(dev), rows=torch.from_numpy(group_rows.view(np.int32)).to(dev))

    def clear_groups(self) -> None:
        self._groups = None

    def _group_tables(self) -> Optional[dict]:
        """the tables of the present rows, None (and stale ones dropped) where there are none"""
        g = self._groups
        if g is not None and g["version"] != self._rows_version():
            g = self._groups = None
        return g

    @property
    def ngroups(self) -> int:
        g = self._group_tables()
        return 0 if g is None else int(g["keys"].numel())

    def _need_groups(self) -> dict:
        self._group_refusal()
        g = self._group_tables()
        if g is None:
            raise RuntimeError(NO_GROUPS.format(type(self).__name__))
        return g

    def search_grouped(self, x, k: int, params=None):
        """x np.ndarray [nq,d] float32 -> (D [nq,k] float32, I [nq,k] int64, G [nq,k] int64) numpy (module docstring).
        params: SearchParameters(sel=...), or SearchParametersIVF(sel=..., nprobe=...) on an inverted-file index, as on `search`."""
        self._need_groups()
        ivf = hasattr(self, "nprobe")
        sel, nprobe = unpack_params(params, ivf=ivf)
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2:
            raise ValueError("search_grouped: x must be 2-D")
        q = torch.from_numpy(x).to(self.device)
        kept = getattr(self, "nprobe", None)
        try:
            if nprobe is not None:
                self.nprobe = nprobe
            D, I, G = self.search_grouped_device(q, int(k), sel=sel)
        finally:
            if ivf:
                self.nprobe = kept
        return D.cpu().numpy(), I.cpu().numpy(), G.cpu().numpy()


def workspace_regions(n: int, N: int, G: int):
    """(offset of best, offset of the merge parts) in the one allocation of wise_group_workspace_bytes for n queries: ord at 0,
    then best, then the parts, each region aligned to 256 bytes (include/wise_hip.h) — the one place Python restates that layout"""
    align = lambda v: (v + 255) // 256 * 256
    best_at = align(4 * n * N)
    return best_at, best_at + align(8 * n * G)


def run(q: torch.Tensor, k: int, tables: dict, scores: Callable, workspace: Callable[[int], torch.Tensor], ids: Optional[torch.Tensor],
        id_base: int, metric: str = "ip", chunk: Optional[int] = None):
    """(D [nq,k], I [nq,k], G [nq,k]) on the device for the queries q [nq, d].
    tables: the index's group tables (GroupTables).  scores(qs, ord): stage 1 for a chunk of queries — the type's *_group_scores call
    into ord, the device address of the chunk's [n][N] uint32 region.  workspace(need): a byte tensor of at least `need` bytes.
    ids / id_base: the rows' external ids.  metric 'l2': D holds distances (the keys order their negation).
    chunk: queries per chunk (default: as many as range_search.WORKSPACE_BYTES allows)."""
    lib = _lib.lib()
    nq, dev, k = q.shape[0], q.device, int(k)
    N, G = int(tables["n"]), int(tables["keys"].numel())
    if k < 1 or k > 2048:
        raise ValueError(f"search_grouped: k={k} out of [1, 2048]")
    D = torch.empty(nq, k, dtype=torch.float32, device=dev)
    I = torch.empty(nq, k, dtype=torch.int64, device=dev)
    Gk = torch.empty(nq, k, dtype=torch.int64, device=dev)
    if nq == 0:
        return D, I, Gk
    one = lib.wise_group_workspace_bytes(N, G, 1, k)
    if one == 0:
        raise ValueError(f"search_grouped: unsupported shape N={N} G={G} k={k}")
    if chunk is None:
        chunk = max(1, min(nq, _range.WORKSPACE_BYTES // one))
    st = _lib.stream_ptr()
    for s in range(0, nq, chunk):
        qs = q[s:s + chunk]
        n = qs.shape[0]
        need = lib.wise_group_workspace_bytes(N, G, n, k)
        if need == 0:
            raise ValueError(f"search_grouped: unsupported shape N={N} G={G} nq={n} k={k}")
        ws = workspace(need)
        best_at, part_at = workspace_regions(n, N, G)
        ord_ptr, best_ptr, part_ptr = ws.data_ptr(), ws.data_ptr() + best_at, ws.data_ptr() + part_at
        scores(qs, ord_ptr)
        _lib.check(lib.wise_group_best(ord_ptr, N, n, tables["off"].data_ptr(), tables["rows"].data_ptr(), G, best_ptr, st), "wise_group_best")
        _lib.check(lib.wise_group_topk(best_ptr, G, n, k, tables["gid"].data_ptr(), N, tables["keys"].data_ptr(), _lib.ptr(ids), int(id_base),
                                       1 if metric == "l2" else 0, D[s:s + n].data_ptr(), I[s:s + n].data_ptr(), Gk[s:s + n].data_ptr(),
                                       part_ptr, ws.numel() - part_at, st), "wise_group_topk")
    return D, I, Gk

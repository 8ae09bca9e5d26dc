"""range_search — "every vector that scores above a threshold" — for the index types whose scan scores are exact functions of
the stored rows: FlatIPIndex, IVFFlatIPIndex, IVFSQIPIndex (faiss's Index::range_search, METRIC_INNER_PRODUCT).

    lims, D, I = index.range_search(x, thresh, params=None)

A row is a hit iff score > thresh, strictly.  lims [nq + 1] int64 with lims[0] = 0; query q's hits are D[lims[q]:lims[q + 1]]
(float32) and I[lims[q]:lims[q + 1]] (int64 external ids), ordered by descending score, ties by ascending row position (the
row of X; the position in list order for the inverted-file types).  faiss promises no order; here it is part of the contract,
so the same index and inputs give the same bytes.  A hit's score is, bit for bit, what the index's fp32 scan gives that row.

What this module holds is the part every type shares: a count / fill pair of the C ABI (include/wise_hip.h) run over chunks of
queries, the one host round trip per chunk (the counts, to size the output), and the ordering of each segment on the device.
The count pass leaves a hit bitmap per query in the workspace — N / 8 bytes per query — so a batch is cut into chunks whose
workspace stays under WORKSPACE_BYTES (256 MiB: 204 queries per chunk at 10M rows; one query per chunk beyond 2^31 rows).
"""
from __future__ import annotations

import math
from typing import Callable, Optional

import numpy as np
import torch

from .. import _lib

WORKSPACE_BYTES = 256 << 20      # bound on the count / fill workspace of one chunk of queries (a chunk holds at least one query)

UNSUPPORTED = ("{}: range_search is not implemented — the scores of the product-quantized types are approximate and their "
               "re-ranking stage would need a contract of its own; FlatIPIndex, IVFFlatIPIndex and IVFSQIPIndex support it")
NO_SHARDED = ("range_search is not implemented on a sharded index: the result is variable-length and the exchange for it is "
              "not built; FlatIPIndex, IVFFlatIPIndex and IVFSQIPIndex on one GPU support it")


def check_threshold(thresh) -> float:
    """The threshold as a Python float; ValueError unless it is a finite number (-3.4028235e38 returns every candidate row)."""
    if isinstance(thresh, bool) or not isinstance(thresh, (int, float, np.integer, np.floating)):
        raise ValueError(f"range_search: thresh must be a finite float, got {type(thresh).__name__}")
    t = float(thresh)
    if not math.isfinite(t) or abs(t) >= 3.4028235677973366e38:      # rounds to a float32 infinity, the type the kernels take it in
        raise ValueError(f"range_search: thresh={thresh!r} must be finite")
    return t


def order_segments(D: torch.Tensor, P: torch.Tensor, counts: torch.Tensor, ascending: bool = False) -> torch.Tensor:
    """The permutation that puts every query's segment of (D, P) — scores and positions as a fill pass wrote them, query after
    query — into descending score, ties by ascending position.  Two device sorts: one of a 64-bit key per hit (the score's bits
    mapped to a signed integer of the same order — -0.0 below +0.0, as the scans' keys have it — above 2^32 - 1 - position), then a
    stable one by query.  Positions are unique within a query, so the order is total and the same on every run.
    ascending (the L2 metric: D holds distances): the same order on the scores -D — negating a float is exact —, that is ascending
    distance, ties by ascending position."""
    total = D.numel()
    bits = (-D if ascending else D).view(torch.int32)
    okey = bits ^ ((bits >> 31) & 0x7FFFFFFF)
    key = (okey.to(torch.int64) << 32) | (0xFFFFFFFF - P)
    qid = torch.repeat_interleave(torch.arange(counts.numel(), device=D.device), counts, output_size=total)
    by_key = torch.sort(key, descending=True).indices
    by_query = torch.sort(qid[by_key], stable=True).indices
    return by_key[by_query]


def run(q: torch.Tensor, workspace_bytes: Callable[[int], int], stage: Callable, workspace: Callable[[int], torch.Tensor],
        ids: Optional[torch.Tensor], id_base: int, chunk: Optional[int] = None, ascending: bool = False):
    """(lims [nq + 1], D, I) on the device for the queries q [nq, d].
    workspace_bytes(n): the *_range_workspace_bytes of n queries (0: unsupported shape).
    stage(qs) -> (count, fill) for a chunk of queries: count(counts, ws) runs the count pass into counts [n] int64, fill(lims, D, P,
    ws) the fill pass with ids == NULL, so that P receives POSITIONS — the tie key; ids are looked up after the ordering.
    chunk: queries per chunk (default: as many as WORKSPACE_BYTES allows).
    ascending: D holds distances (the L2 metric); every segment comes by ascending distance (order_segments)."""
    nq, dev = q.shape[0], q.device
    lims = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    Ds, Ps = [], []
    if nq:
        one = workspace_bytes(1)
        if one == 0:
            raise ValueError("range_search: unsupported shape")
        if chunk is None:
            chunk = max(1, min(nq, WORKSPACE_BYTES // one))
    base = 0
    for s in range(0, nq, chunk or 1):
        qs = q[s:s + chunk]
        n = qs.shape[0]
        need = workspace_bytes(n)
        if need == 0:
            raise ValueError(f"range_search: unsupported shape nq={n}")
        ws = workspace(need)
        count, fill = stage(qs)
        counts = torch.empty(n, dtype=torch.int64, device=dev)
        count(counts, ws)
        sub = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(counts, 0, out=sub[1:])
        total = int(sub[-1].item())          # the host round trip: the output is sized from the counts
        lims[s + 1:s + n + 1] = sub[1:] + base
        base += total
        if total == 0:
            continue
        D = torch.empty(total, dtype=torch.float32, device=dev)
        P = torch.empty(total, dtype=torch.int64, device=dev)
        fill(sub, D, P, ws)
        perm = order_segments(D, P, counts, ascending)
        Ds.append(D[perm])
        Ps.append(P[perm])
    if not Ds:
        return lims, torch.empty(0, dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.int64, device=dev)
    D, P = (Ds[0], Ps[0]) if len(Ds) == 1 else (torch.cat(Ds), torch.cat(Ps))
    return lims, D, (ids[P] if ids is not None else P + int(id_base))


def to_numpy(x) -> torch.Tensor:
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("range_search: x must be 2-D")
    return torch.from_numpy(x)

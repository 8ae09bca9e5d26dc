"""Filtered search (IDSelector, wise_amd/index/selector.py) beside the unfiltered search on the same rows, the same box, the same
run ("Search restricted to a set of ids").

A seeded clustered set is generated on the device as in tools/ivfpq_bench.py; an IndexFlatIP (no shadow copies: the filtered
search is the fp32 scan, and it is set beside the unfiltered fp32 scan), an IndexIVFFlat and an IndexIVFPQ<m> hold the same rows
(the PQ index takes the flat IVF index's centroids).  For the selectivities 1, 0.1, 0.01 and 0.001 of the rows — a seeded batch of
that many ids — and nq in {1, 256}, k = 10, whole `search_device` calls are timed with HIP events, the selector already resolved.
Reported per point: queries/s of the filtered and of the unfiltered search of the three indexes, the seconds it takes to resolve
a batch selector of that size from scratch (sort and de-duplicate, bitmap, and for the flat index the position list), and the
bytes the flat scan reads, n_pos * d * 4, with the seconds per byte of the filtered and the unfiltered fp32 scan beside it: the
sanity condition is that filtered flat search at selectivity s reads about s * N * d * 4 bytes, i.e. that its time per search
falls with s until launch overhead takes over.

    timeout 1100 python tools/sel_bench.py [--rows 10000000] [--dim 512] [--m 64] [--nprobe 32] [--iters 10] [--out FILE]

One GPU process: run it under a time limit of its own, as above.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from wise_amd.index.flat_ip import FlatIPIndex  # noqa: E402
from wise_amd.index.ivf_flat import IVFFlatIPIndex, reference_nlist  # noqa: E402
from wise_amd.index.ivf_pq import IVFPQIPIndex  # noqa: E402
from wise_amd.index.selector import IDSelectorBatch  # noqa: E402

SELECTIVITIES = (1.0, 0.1, 0.01, 0.001)


def rows_chunk(centres, n, noise, g):
    pick = torch.randint(0, centres.shape[0], (n,), generator=g, device="cuda")
    x = centres[pick] + noise * torch.nn.functional.normalize(torch.randn(n, centres.shape[1], generator=g, device="cuda"), dim=1)
    return torch.nn.functional.normalize(x, dim=1)


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters / 1e3


def resolve_seconds(ids, index, positions, repeats=3):
    """Wall seconds to resolve a fresh batch selector over `ids` against `index` (nothing cached), the best of `repeats`."""
    best = float("inf")
    for _ in range(repeats):
        sel = IDSelectorBatch(ids)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = sel.resolve(index)
        if positions:
            res.positions()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--noise", type=float, default=0.35)
    ap.add_argument("--out", default="sel_bench.json")
    args = ap.parse_args()
    N, d, m, k = args.rows, args.dim, args.m, 10
    nlist = reference_nlist(N)
    g = torch.Generator(device="cuda").manual_seed(0)
    centres = torch.nn.functional.normalize(torch.randn(max(nlist // 2, 16), d, generator=g, device="cuda"), dim=1)
    chunk = 1 << 20
    t0 = time.time()
    ivf, pq = IVFFlatIPIndex(d, nlist), IVFPQIPIndex(d, nlist, m)
    train = rows_chunk(centres, min(N, 100 * nlist), args.noise, g)
    ivf.train(train)
    pq.set_centroids(ivf.centroids)
    pq.codebooks = pq.train_codebooks(pq.training_residuals(train))
    del train
    g = torch.Generator(device="cuda").manual_seed(1)
    Q = None
    for s in range(0, N, chunk):
        x = rows_chunk(centres, min(chunk, N - s), args.noise, g)
        ids = torch.arange(s, s + x.shape[0], dtype=torch.int64, device="cuda")
        ivf.add_with_ids(x, ids)
        pq.add_with_ids(x, ids)
        if Q is None:      # queries: perturbed rows of the set
            Q = torch.nn.functional.normalize(x[:256] + 0.05 * torch.nn.functional.normalize(torch.randn(256, d, generator=g, device="cuda"), dim=1), dim=1).contiguous()
    ivf._finalize()
    pq._finalize()
    ivf.nprobe = pq.nprobe = args.nprobe
    # the flat index over the same rows, in list order, under the same ids; no shadow: fp32 scan beside fp32 scan
    flat = FlatIPIndex(d, shadow=False).adopt(ivf._lists.data, ivf._lists.ids)
    torch.cuda.synchronize()
    print(f"{N} x {d}, nlist {nlist}, m {m}, nprobe {args.nprobe}: built in {time.time() - t0:.1f} s", flush=True)
    indexes = (("IndexFlatIP", flat), ("IndexIVFFlat", ivf), (f"IndexIVFPQ{m}", pq))
    res = {"rows": N, "dim": d, "nlist": nlist, "m": m, "k": k, "nprobe": args.nprobe, "iters": args.iters,
           "device": torch.cuda.get_device_name(0), "unfiltered": [], "points": []}
    plain = {}
    for nq in (1, 256):
        q = Q[:nq].contiguous()
        point = {"nq": nq}
        for name, idx in indexes:
            t = timed(lambda: idx.search_device(q, k), args.iters)
            plain[(name, nq)] = t
            point[name] = {"seconds_per_search": t, "queries_per_s": nq / t}
        print(json.dumps(point), flush=True)
        res["unfiltered"].append(point)
    full_bytes = N * d * 4
    rng = np.random.default_rng(2)
    for s in SELECTIVITIES:
        n_sel = max(int(round(N * s)), 1)
        chosen = rng.permutation(N)[:n_sel].astype(np.int64)
        sel = IDSelectorBatch(chosen)
        n_pos = int(sel.resolve(flat).positions().numel())
        for _, idx in indexes[1:]:
            sel.resolve(idx)
        resolve = {"IndexFlatIP": resolve_seconds(chosen, flat, True), "IndexIVFFlat": resolve_seconds(chosen, ivf, False)}
        for nq in (1, 256):
            q = Q[:nq].contiguous()
            point = {"selectivity": s, "selected_rows": n_pos, "nq": nq, "resolve_batch_seconds": resolve,
                     "flat_scan_bytes": n_pos * d * 4, "flat_scan_bytes_unfiltered": full_bytes}
            for name, idx in indexes:
                t = timed(lambda: idx.search_device(q, k, sel=sel), args.iters)
                point[name] = {"seconds_per_search": t, "queries_per_s": nq / t, "unfiltered_queries_per_s": nq / plain[(name, nq)]}
            tf, tu = point["IndexFlatIP"]["seconds_per_search"], plain[("IndexFlatIP", nq)]
            # filtered flat search reads about s * N * d * 4 bytes: its time against the unfiltered fp32 scan's, beside the byte ratio
            point["flat_sanity"] = {"bytes_ratio": n_pos / N, "seconds_ratio": tf / tu}
            print(json.dumps(point), flush=True)
            res["points"].append(point)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()

"""range_search beside the same index's top-10 search, same rows, same box, same run ("range_search").

One seeded clustered set on the device (tools/ivfsq_bench.py's recipe), one coarse k-means shared by IndexIVFFlat and IndexIVFSQ8,
an exhaustive flat index over the same rows.  Thresholds come from the data: the exact scores of a few queries against every row
give the scores that about 10, about 1,000 and about 100,000 rows per query exceed.  Per point (index, nprobe, nq, threshold):
  range_ms      `range_search_device`, one HIP-event pair per call: median, min, max of --iters calls after 3 warm-up calls
  topk10_ms     the same index's `search_device` at k = 10, timed the same way in the same run: the yardstick
  hits_per_query  what the call returned (the inverted-file types return the hits of the probed lists)
  bytes         algorithmic = the candidate rows once (N or the probed lists' rows, times the row's bytes); modelled = what the two
                passes read by construction: the count pass reads the candidate rows once per query tile (flat: ceil(nq / tile)
                passes, tile = 4 at d <= 512; inverted-file: each query its own lists), the fill pass the hit rows again, plus the
                hit bitmap written and read.  A model, not a counter.
No ratio is fixed in advance; the file records what the run gave.

    timeout 1100 python tools/range_bench.py [--rows 10000000] [--dim 512] [--out profiles/range_bench.json]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from wise_amd.index.flat_ip import FlatIPIndex  # noqa: E402
from wise_amd.index.ivf_common import CoarseQuantizer  # noqa: E402
from wise_amd.index.ivf_flat import IVFFlatIPIndex, reference_nlist  # noqa: E402
from wise_amd.index.ivf_sq import IVFSQIPIndex  # noqa: E402

NPROBES = (32, 1024)
TARGETS = (10, 1000, 100000)


def chunk(centres, noise, n, g):
    d = centres.shape[1]
    pick = torch.randint(0, centres.shape[0], (n,), generator=g, device="cuda")
    z = torch.nn.functional.normalize(torch.randn(n, d, generator=g, device="cuda"), dim=1)
    return torch.nn.functional.normalize(centres[pick] + noise * z, dim=1).contiguous()


def timed_ms(fn, iters, warmup=3):
    """median / min / max milliseconds of `iters` calls, each between its own pair of events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms)), "calls": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--noise", type=float, default=0.35)
    ap.add_argument("--out", default="profiles/range_bench.json")
    args = ap.parse_args()
    if args.iters < 10:
        raise SystemExit("--iters: at least 10 timed calls per point")
    N, d = args.rows, args.dim
    nlist = reference_nlist(N)
    g = torch.Generator(device="cuda").manual_seed(0)
    centres = torch.nn.functional.normalize(torch.randn(max(nlist // 2, 16), d, generator=g, device="cuda"), dim=1)
    g = torch.Generator(device="cuda").manual_seed(1)
    train = chunk(centres, args.noise, min(N, 100 * nlist), g)
    coarse = CoarseQuantizer(d, nlist)
    coarse.train(train)
    ivf, sq8 = IVFFlatIPIndex(d, nlist), IVFSQIPIndex(d, nlist)
    ivf.set_centroids(coarse.centroids)
    sq8.set_centroids(coarse.centroids)
    resid = sq8._residuals(train, sq8._coarse.assign_device(train, sq8.centroids))
    sq8.set_trained(resid.amin(dim=0), resid.amax(dim=0) - resid.amin(dim=0))
    del train, resid
    flat, Q = FlatIPIndex(d), None
    flat.reserve(N)
    g = torch.Generator(device="cuda").manual_seed(2)
    for s in range(0, N, 1 << 20):
        x = chunk(centres, args.noise, min(1 << 20, N - s), g)
        ids = torch.arange(s, s + x.shape[0], dtype=torch.int64, device="cuda")
        for i in (flat, ivf, sq8):
            i.add_with_ids(x, ids)
        if Q is None:      # queries: perturbed rows of the set
            Q = torch.nn.functional.normalize(x[:256] + 0.05 * torch.nn.functional.normalize(torch.randn(256, d, generator=g, device="cuda"), dim=1), dim=1).contiguous()
    for i in (flat, ivf, sq8):
        i._finalize()
        torch.cuda.empty_cache()
    # thresholds from the data: exact scores of 8 queries against every row
    scores = Q[:8] @ flat._X.T
    thresholds = {}
    for want in TARGETS:
        kth = min(want, N - 1)
        thresholds[want] = float(torch.topk(scores, kth + 1, dim=1).values[:, kth].median())
    del scores
    out = {"device": torch.cuda.get_device_name(0), "rows": N, "dim": d, "nlist": nlist, "iters": args.iters, "noise": args.noise,
           "thresholds": {str(k): v for k, v in thresholds.items()}, "points": []}
    tile = max(1, min(4, 8 // ((d // 4 + 63) // 64)))
    plans = [("IndexFlatIP", flat, None, 4 * d)] + [(n, i, p, w) for p in NPROBES for n, i, w in (("IndexIVFFlat", ivf, 4 * d), ("IndexIVFSQ8", sq8, d))]
    for name, index, nprobe, row_bytes in plans:
        if nprobe is not None:
            index.nprobe = nprobe
        for nq in (1, 256):
            q = Q[:nq].contiguous()
            topk = timed_ms(lambda: index.search_device(q, 10), args.iters)
            if nprobe is None:
                cand = float(N)
            else:
                probes = index.probes_device(q, index._clamped_nprobe())
                off = index._lists.list_off
                cand = float((off[probes + 1] - off[probes]).sum().item()) / nq
            for want, t in thresholds.items():
                lims, _, _ = index.range_search_device(q, t)
                hits = float(lims[-1].item()) / nq
                rng = timed_ms(lambda: index.range_search_device(q, t), args.iters)
                passes = -(-nq // min(tile, nq)) / nq if nprobe is None else 1.0     # reads of the candidate rows per query
                point = {"index": name, "nprobe": nprobe, "nq": nq, "target_hits": want, "threshold": t, "hits_per_query": hits,
                         "range_ms": rng, "topk10_ms": topk, "range_over_topk10": rng["median"] / topk["median"],
                         "bytes": {"algorithmic_per_query": cand * row_bytes,
                                   "modelled_per_query": cand * row_bytes * passes + hits * row_bytes + 2 * cand / 8}}
                print(json.dumps(point), flush=True)
                out["points"].append(point)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()

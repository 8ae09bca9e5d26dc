"""IndexIVFSQfp16 beside IndexIVFFlat and IndexIVFSQ8 on the same rows, the same coarse quantizer, the same box, the same run
(DESIGN.md §4): bytes held, queries/s, the second stage alone and recall@10 against the exhaustive answer.

One seeded clustered set is generated on the device (tools/ivfsq_bench.py's recipe).  One coarse k-means; the three indexes take
its centroids.  Reported per index: HBM bytes, add seconds, and per nprobe in {32, 1024} recall@10, and for nq in {1, 256} the
time of whole `search_device` calls and of the second stage alone (the probes computed once and handed back to the index, so what
is timed is everything after the coarse stage).  Timing: every shape of every index is warmed up first; then the three indexes
ALTERNATE — round r times one call of each, HIP events around the single call — for --iters rounds (at least 10), so that clock
and thermal drift fall on all three alike; a point reports the median with the smallest and the largest call (the spread).
The ratios second stage IndexIVFSQfp16 / IndexIVFFlat are reported next to the byte ratio (2 d + 8) / (4 d + 8): the scan reads
half the bytes per row, so the expectation is a ratio below 1 at nq = 256, nprobe 1024.  No value is fixed in advance; if the
expectation does not hold, tools/pmc_sq.py gives the bytes per launch in a counter pass of its own.

    timeout 1100 python tools/ivfsqfp16_bench.py [--rows 10000000] [--dim 512] [--out profiles/ivfsqfp16_bench.json]

One GPU process: run it under a time limit of its own, as above.  At 10M x 512 the three indexes and the fp32 rows kept for the
exhaustive answer take about 57 GB of HBM, and merging IndexIVFFlat's lists needs about 40 GB more for a moment.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from wise_amd import _lib  # noqa: E402
from wise_amd.index.flat_ip import FlatIPIndex  # noqa: E402
from wise_amd.index.ivf_common import CoarseQuantizer  # noqa: E402
from wise_amd.index.ivf_flat import IVFFlatIPIndex, reference_nlist  # noqa: E402
from wise_amd.index.ivf_sq import IVFSQfp16IPIndex, IVFSQIPIndex  # noqa: E402

NPROBES = (32, 1024)
NQS = (1, 256)


def chunk(centres, noise, n, g):
    d = centres.shape[1]
    pick = torch.randint(0, centres.shape[0], (n,), generator=g, device="cuda")
    z = torch.nn.functional.normalize(torch.randn(n, d, generator=g, device="cuda"), dim=1)
    return torch.nn.functional.normalize(centres[pick] + noise * z, dim=1).contiguous()


def one_call_seconds(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def alternate(fns: dict, iters: int, warmup: int = 2) -> dict:
    """name -> {median, min, max} seconds of one call, the callables taking turns round by round"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(iters):
        for name, fn in fns.items():
            times[name].append(one_call_seconds(fn))
    return {name: {"median": statistics.median(t), "min": min(t), "max": max(t)} for name, t in times.items()}


def recall(I, If):
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / len(b) for a, b in zip(I, If)]))


def clock():
    torch.cuda.synchronize()
    return time.time()


def held_bytes(index):
    """HBM bytes of the merged index (IndexIVFFlat has no hbm_bytes(): its lists and its centroids)"""
    if hasattr(index, "hbm_bytes"):
        return index.hbm_bytes()
    return index._lists.nbytes() + index.centroids.numel() * index.centroids.element_size()


class FixedProbes:
    """search_device with the coarse stage's answer computed once and handed back: the time of everything after it"""

    def __init__(self, index, q, k):
        self.index, self.q, self.k = index, q, k
        self.probes = index.probes_device(q, index._clamped_nprobe()).contiguous()

    def __call__(self):
        coarse = self.index._coarse
        real = coarse.probes_device
        coarse.probes_device = lambda qs, nprobe: self.probes
        try:
            return self.index.search_device(self.q, self.k)
        finally:
            coarse.probes_device = real


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--noise", type=float, default=0.35)
    ap.add_argument("--out", default="profiles/ivfsqfp16_bench.json")
    args = ap.parse_args()
    if args.iters < 10:
        ap.error("--iters: at least 10 timed calls per point")
    N, d, k = args.rows, args.dim, 10
    nlist = reference_nlist(N)
    g = torch.Generator(device="cuda").manual_seed(0)
    centres = torch.nn.functional.normalize(torch.randn(max(nlist // 2, 16), d, generator=g, device="cuda"), dim=1)
    g = torch.Generator(device="cuda").manual_seed(1)
    train = chunk(centres, args.noise, min(N, 100 * nlist), g)
    names = ["IndexIVFFlat", "IndexIVFSQ8", "IndexIVFSQfp16"]
    idx = dict(zip(names, (IVFFlatIPIndex(d, nlist), IVFSQIPIndex(d, nlist), IVFSQfp16IPIndex(d, nlist))))
    t0 = clock()
    coarse = CoarseQuantizer(d, nlist)
    coarse.train(train)
    t_coarse = clock() - t0
    for i in idx.values():
        i.set_centroids(coarse.centroids)
    flat, sq8, sq16 = (idx[n] for n in names)
    resid = sq8._residuals(train, sq8._coarse.assign_device(train, sq8.centroids))
    trained = torch.empty(2 * d, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().wise_sq_train(resid.data_ptr(), resid.shape[0], d, trained.data_ptr(), _lib.stream_ptr()), "wise_sq_train")
    sq8.trained = trained
    del train, resid
    print(f"{N} x {d}, nlist {nlist}: coarse {t_coarse:.1f} s", flush=True)
    exact, add_s, Q = FlatIPIndex(d), dict.fromkeys(names, 0.0), None
    exact.reserve(N)
    g = torch.Generator(device="cuda").manual_seed(2)
    for s in range(0, N, 1 << 20):
        x = chunk(centres, args.noise, min(1 << 20, N - s), g)
        ids = torch.arange(s, s + x.shape[0], dtype=torch.int64, device="cuda")
        exact.add_with_ids(x, ids)
        for name, i in idx.items():
            t0 = clock()
            i.add_with_ids(x, ids)
            add_s[name] += clock() - t0
        if Q is None:      # queries: perturbed rows of the set
            Q = torch.nn.functional.normalize(x[:256] + 0.05 * torch.nn.functional.normalize(torch.randn(256, d, generator=g, device="cuda"), dim=1), dim=1).contiguous()
    for name, i in idx.items():
        t0 = clock()
        i._finalize()
        add_s[name] += clock() - t0
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "rows": N, "dim": d, "nlist": nlist, "k": k, "iters": args.iters, "noise": args.noise,
           "timing": "the three indexes alternate call by call; seconds of one call: median, min, max over iters calls",
           "train_seconds": {"coarse_kmeans": t_coarse}, "add_seconds": add_s,
           "hbm_bytes": {name: held_bytes(i) for name, i in idx.items()}, "points": []}
    _, If = exact.search_device(Q, k)
    If = If.cpu().numpy()
    for nprobe in NPROBES:
        for i in idx.values():
            i.nprobe = nprobe
        rec = {name: recall(i.search_device(Q, k)[1].cpu().numpy(), If) for name, i in idx.items()}
        for nq in NQS:
            q = Q[:nq].contiguous()
            whole = alternate({name: (lambda i=i: i.search_device(q, k)) for name, i in idx.items()}, args.iters)
            stage2 = alternate({name: FixedProbes(i, q, k) for name, i in idx.items()}, args.iters)
            for name in names:
                point = {"index": name, "nprobe": nprobe, "nq": nq, "recall_at_10": rec[name], "search_seconds": whole[name],
                         "queries_per_s": nq / whole[name]["median"], "second_stage_seconds": stage2[name]}
                print(json.dumps(point), flush=True)
                out["points"].append(point)
            for other in names[:2]:
                out[f"second_stage_time_ratio_sqfp16_over_{other[5:].lower()}_nprobe{nprobe}_nq{nq}"] = \
                    stage2[names[2]]["median"] / stage2[other]["median"]
    out["bytes_ratio_sqfp16_over_ivfflat"] = (2 * d + 8) / (4 * d + 8)
    out["bytes_ratio_sqfp16_over_sq8"] = (2 * d + 8) / (d + 8)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({k_: v for k_, v in out.items() if k_.startswith(("second_stage", "bytes_ratio", "hbm"))}))
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()

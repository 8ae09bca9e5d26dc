"""IndexIVFSQ8 beside IndexIVFFlat and IndexIVFPQ<m>R8 on the same rows, the same coarse quantizer, the same box, the same run
(DESIGN.md §4): bytes held, queries/s and recall@10 against the exhaustive answer.

One seeded clustered set is generated on the device (tools/ivfpq_bench.py's recipe: unit rows around random unit centres,
isotropic noise).  One coarse k-means; the three indexes take its centroids.  Reported per index: HBM bytes, add seconds, and per
nprobe in {32, 1024} recall@10 and queries/s at nq in {1, 256} with HIP events around whole `search_device` calls.  For
IndexIVFSQ8 and IndexIVFFlat also the time of the second stage alone at nq = 1 (the probes computed once and handed back to the
index, so what is timed is everything after the coarse stage), and the ratio of the two at nprobe 1024: the scan reads
(d + 8) / (4 d + 8) of the bytes, so the expectation is a ratio below 1.  No value is fixed in advance.

    timeout 1100 python tools/ivfsq_bench.py [--rows 10000000] [--dim 512] [--m 64] [--out profiles/ivfsq_bench.json]

One GPU process: run it under a time limit of its own, as above.  At 10M x 512 the three indexes and the fp32 rows kept for the
exhaustive answer take about 52 GB of HBM, and merging IndexIVFFlat's lists needs about 40 GB more for a moment.
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
from wise_amd import _lib  # noqa: E402
from wise_amd.index.flat_ip import FlatIPIndex  # noqa: E402
from wise_amd.index.ivf_common import CoarseQuantizer  # noqa: E402
from wise_amd.index.ivf_flat import IVFFlatIPIndex, reference_nlist  # noqa: E402
from wise_amd.index.ivf_pq import IVFPQRefineIPIndex  # noqa: E402
from wise_amd.index.ivf_sq import IVFSQIPIndex  # noqa: E402

NPROBES = (32, 1024)


def chunk(centres, noise, n, g):
    d = centres.shape[1]
    pick = torch.randint(0, centres.shape[0], (n,), generator=g, device="cuda")
    z = torch.nn.functional.normalize(torch.randn(n, d, generator=g, device="cuda"), dim=1)
    return torch.nn.functional.normalize(centres[pick] + noise * z, dim=1).contiguous()


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


def second_stage_seconds(index, q, k, iters):
    """search_device with the coarse stage's answer computed once and handed back: the time of everything after it"""
    probes = index.probes_device(q, index._clamped_nprobe()).contiguous()
    coarse = index._coarse
    real = coarse.probes_device
    coarse.probes_device = lambda qs, nprobe: probes
    try:
        return timed(lambda: index.search_device(q, k), iters)
    finally:
        coarse.probes_device = real


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--noise", type=float, default=0.35)
    ap.add_argument("--out", default="profiles/ivfsq_bench.json")
    args = ap.parse_args()
    N, d, m, k = args.rows, args.dim, args.m, 10
    nlist = reference_nlist(N)
    g = torch.Generator(device="cuda").manual_seed(0)
    centres = torch.nn.functional.normalize(torch.randn(max(nlist // 2, 16), d, generator=g, device="cuda"), dim=1)
    g = torch.Generator(device="cuda").manual_seed(1)
    train = chunk(centres, args.noise, min(N, 100 * nlist), g)
    names = ["IndexIVFFlat", "IndexIVFSQ8", f"IndexIVFPQ{m}R8"]
    idx = dict(zip(names, (IVFFlatIPIndex(d, nlist), IVFSQIPIndex(d, nlist), IVFPQRefineIPIndex(d, nlist, m, 8))))
    t0 = clock()
    coarse = CoarseQuantizer(d, nlist)
    coarse.train(train)
    t_coarse = clock() - t0
    for i in idx.values():
        i.set_centroids(coarse.centroids)
    flat, sq8, pq = (idx[n] for n in names)
    t0 = clock()
    resid = pq.training_residuals(train)
    pq.codebooks = pq.train_codebooks(resid)
    t_pq = clock() - t0
    del resid
    t0 = clock()
    resid = sq8._residuals(train, sq8._coarse.assign_device(train, sq8.centroids))
    vmin, vmax = resid.amin(dim=0), resid.amax(dim=0)           # (checked against the trainer below)
    trained = torch.empty(2 * d, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().wise_sq_train(resid.data_ptr(), resid.shape[0], d, trained.data_ptr(), _lib.stream_ptr()), "wise_sq_train")
    sq8.trained = trained
    t_sq = clock() - t0
    assert torch.equal(trained[:d], vmin) and torch.equal(trained[d:], vmax - vmin)
    del train, resid
    print(f"{N} x {d}, nlist {nlist}: coarse {t_coarse:.1f} s, PQ codebooks {t_pq:.1f} s, SQ ranges {t_sq:.2f} s", flush=True)
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
    out = {"device": torch.cuda.get_device_name(0), "rows": N, "dim": d, "nlist": nlist, "m": m, "k": k, "iters": args.iters,
           "noise": args.noise, "k_factor": pq.k_factor,
           "train_seconds": {"coarse_kmeans": t_coarse, names[2]: t_pq, names[1]: t_sq}, "add_seconds": add_s,
           "hbm_bytes": {name: held_bytes(i) for name, i in idx.items()}, "points": []}
    _, If = exact.search_device(Q, k)
    If = If.cpu().numpy()
    stage2 = {}
    for nprobe in NPROBES:
        for name, i in idx.items():
            i.nprobe = nprobe
            point = {"index": name, "nprobe": nprobe, "recall_at_10": recall(i.search_device(Q, k)[1].cpu().numpy(), If)}
            for nq in (1, 256):
                q = Q[:nq].contiguous()
                point[f"queries_per_s_nq{nq}"] = nq / timed(lambda: i.search_device(q, k), args.iters)
            if i is not pq:
                point["second_stage_seconds_nq1"] = stage2[name, nprobe] = second_stage_seconds(i, Q[:1].contiguous(), k, args.iters)
            print(json.dumps(point), flush=True)
            out["points"].append(point)
    for nprobe in NPROBES:
        out[f"second_stage_time_ratio_sq8_over_ivfflat_nprobe{nprobe}_nq1"] = stage2[names[1], nprobe] / stage2[names[0], nprobe]
    out["bytes_ratio_sq8_over_ivfflat"] = (d + 8) / (4 * d + 8)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({k_: v for k_, v in out.items() if k_.startswith(("second_stage", "bytes_ratio", "hbm"))}))
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()

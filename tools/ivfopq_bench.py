"""IndexIVFOPQ<m> beside IndexIVFPQ<m>, and their R8 forms, on the same rows, the same coarse quantizer, the same box, the same
run: what the learned rotation buys in recall and what it costs in time.

Two seeded sets are generated on the device, each searched by all four indexes:
  clustered   tools/ivfpq_bench.py's set: unit rows around random unit centres, isotropic noise
  decaying    the recipe of the CPU study behind tests/golden/ivfopq_quality.json, scaled: a row's offset from its centre has
              per-coordinate deviation proportional to 1 / sqrt(1 + i), turned by a seeded random orthogonal matrix
One coarse k-means per set; IndexIVFPQ<m> and IndexIVFOPQ<m> take its centroids and train on the residuals of the same training
sample (the R8 forms share their trained state: same codebooks, same rotation, plus the compact rows).  Reported per set:
training seconds (codebooks alone / rotation + codebooks), add seconds per index, recall@10 against the exhaustive answer per
nprobe, queries/s at nq in {1, 256} with HIP events around whole `search_device` calls, and for the R8 forms the same per
k_factor in {1, 2, 5, 10, 20, 50}.

    timeout 1100 python tools/ivfopq_bench.py [--rows 10000000] [--dim 512] [--m 64] [--sets clustered,decaying] [--out FILE]

One GPU process: run it under a time limit of its own, as above.  At 10M x 512 the four indexes and the fp32 rows kept for the
exhaustive answer take about 33 GB of HBM per set.
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
from wise_amd.index.ivf_flat import reference_nlist  # noqa: E402
from wise_amd.index.ivf_common import CoarseQuantizer  # noqa: E402
from wise_amd.index.ivf_pq import IVFOPQIPIndex, IVFOPQRefineIPIndex, IVFPQIPIndex, IVFPQRefineIPIndex  # noqa: E402

K_FACTORS = (1, 2, 5, 10, 20, 50)
NPROBES = (32, 1024)


class RowSource:
    """Seeded rows of one of the two sets, a chunk at a time."""

    def __init__(self, kind, d, centres, noise, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.kind, self.noise = kind, noise
        self.centres = torch.nn.functional.normalize(torch.randn(centres, d, generator=g, device="cuda"), dim=1)
        if kind == "decaying":
            s = 1.0 / torch.sqrt(1.0 + torch.arange(d, dtype=torch.float32, device="cuda"))
            self.scale = s * (noise / torch.sqrt((s * s).sum()))
            q, r = torch.linalg.qr(torch.randn(d, d, generator=g, device="cuda"))
            self.mix = (q * torch.sign(torch.diagonal(r))).contiguous()

    def chunk(self, n, g):
        d = self.centres.shape[1]
        pick = torch.randint(0, self.centres.shape[0], (n,), generator=g, device="cuda")
        z = torch.randn(n, d, generator=g, device="cuda")
        off = (z * self.scale) @ self.mix.t() if self.kind == "decaying" else self.noise * torch.nn.functional.normalize(z, dim=1)
        return torch.nn.functional.normalize(self.centres[pick] + off, dim=1).contiguous()


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


def run_set(kind, args):
    N, d, m, k = args.rows, args.dim, args.m, 10
    nlist = reference_nlist(N)
    src = RowSource(kind, d, max(nlist // 2, 16), args.noise if kind == "clustered" else args.decaying_noise, seed=0)
    g = torch.Generator(device="cuda").manual_seed(1)
    train = src.chunk(min(N, 100 * nlist), g)
    names = [f"IndexIVFPQ{m}", f"IndexIVFOPQ{m}", f"IndexIVFPQ{m}R8", f"IndexIVFOPQ{m}R8"]
    idx = dict(zip(names, (IVFPQIPIndex(d, nlist, m), IVFOPQIPIndex(d, nlist, m), IVFPQRefineIPIndex(d, nlist, m, 8),
                           IVFOPQRefineIPIndex(d, nlist, m, 8))))
    t0 = clock()
    coarse = CoarseQuantizer(d, nlist)
    coarse.train(train)
    t_coarse = clock() - t0
    for i in idx.values():
        i.set_centroids(coarse.centroids)
    pq, opq = idx[names[0]], idx[names[1]]
    resid = pq.training_residuals(train)
    t0 = clock()
    pq.codebooks = pq.train_codebooks(resid)
    t_pq = clock() - t0
    t0 = clock()
    opq.rotation, opq.codebooks = opq.train_rotation(resid)
    t_opq = clock() - t0
    idx[names[2]].codebooks = pq.codebooks
    idx[names[3]].codebooks, idx[names[3]].rotation = opq.codebooks, opq.rotation
    del train, resid
    print(f"[{kind}] {N} x {d}, nlist {nlist}, m {m}: coarse {t_coarse:.1f} s, codebooks {t_pq:.1f} s, rotation + codebooks {t_opq:.1f} s", flush=True)
    exact, add_s, Q = FlatIPIndex(d), dict.fromkeys(names, 0.0), None
    exact.reserve(N)
    g = torch.Generator(device="cuda").manual_seed(2)
    for s in range(0, N, 1 << 20):
        x = src.chunk(min(1 << 20, N - s), g)
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
    res = {"set": kind, "rows": N, "dim": d, "nlist": nlist, "m": m, "k": k, "iters": args.iters,
           "train_seconds": {"coarse_kmeans": t_coarse, names[0]: t_pq, names[1]: t_opq}, "add_seconds": add_s,
           "hbm_bytes": {name: i.hbm_bytes() for name, i in idx.items()}, "points": [], "refine_points": []}
    _, If = exact.search_device(Q, k)
    If = If.cpu().numpy()
    for nprobe in NPROBES:
        for name in names[:2]:
            idx[name].nprobe = nprobe
            point = {"index": name, "nprobe": nprobe, "recall_at_10": recall(idx[name].search_device(Q, k)[1].cpu().numpy(), If)}
            for nq in (1, 256):
                q = Q[:nq].contiguous()
                t = timed(lambda: idx[name].search_device(q, k), args.iters)
                point[f"queries_per_s_nq{nq}"] = nq / t
            print(json.dumps(point), flush=True)
            res["points"].append(point)
        for name in names[2:]:
            idx[name].nprobe = nprobe
            for kf in K_FACTORS:
                idx[name].k_factor = kf
                point = {"index": name, "nprobe": nprobe, "k_factor": kf,
                         "recall_at_10": recall(idx[name].search_device(Q, k)[1].cpu().numpy(), If)}
                for nq in (1, 256):
                    q = Q[:nq].contiguous()
                    t = timed(lambda: idx[name].search_device(q, k), args.iters)
                    point[f"queries_per_s_nq{nq}"] = nq / t
                print(json.dumps(point), flush=True)
                res["refine_points"].append(point)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--noise", type=float, default=0.35)
    ap.add_argument("--decaying-noise", type=float, default=0.6)
    ap.add_argument("--sets", default="clustered,decaying")
    ap.add_argument("--out", default="ivfopq_bench.json")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "sets": []}
    for kind in args.sets.split(","):
        out["sets"].append(run_set(kind, args))
        torch.cuda.empty_cache()
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()

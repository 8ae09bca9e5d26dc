"""IndexIVFPQ<m> beside IndexIVFFlat on the same rows, the same coarse quantizer, the same box, the same run.

A seeded clustered set (unit rows around random unit centres) is generated on the device, an IndexIVFFlat is trained and
filled, and an IndexIVFPQ<m> takes the SAME centroids (set_centroids), trains its codebooks on the residuals of the same
training sample and encodes the same rows.  Then both are searched at nq in {1, 256}, nprobe in {32, 1024}, k = 10, timed
with HIP events around whole `search_device` calls (coarse stage included, tables and bias included for the PQ index).
Reported: queries/s, bytes of HBM each index holds, recall@10 of both against the exhaustive answer over the same rows.

    timeout 1100 python tools/ivfpq_bench.py [--rows 10000000] [--dim 512] [--m 64] [--iters 10] [--out FILE]

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


def recall(I, If):
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / len(b) for a, b in zip(I, If)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--noise", type=float, default=0.35)
    ap.add_argument("--out", default="ivfpq_bench.json")
    args = ap.parse_args()
    N, d, m, k = args.rows, args.dim, args.m, 10
    nlist = reference_nlist(N)
    g = torch.Generator(device="cuda").manual_seed(0)
    centres = torch.nn.functional.normalize(torch.randn(max(nlist // 2, 16), d, generator=g, device="cuda"), dim=1)
    chunk = 1 << 20
    t0 = time.time()
    flat, pq = IVFFlatIPIndex(d, nlist), IVFPQIPIndex(d, nlist, m)
    train = rows_chunk(centres, min(N, 100 * nlist), args.noise, g)
    flat.train(train)
    torch.cuda.synchronize()
    t_coarse = time.time() - t0
    pq.set_centroids(flat.centroids)
    pq.codebooks = pq.train_codebooks(pq.training_residuals(train))
    torch.cuda.synchronize()
    t_pq = time.time() - t0 - t_coarse
    del train
    g = torch.Generator(device="cuda").manual_seed(1)
    Q = None
    for s in range(0, N, chunk):
        x = rows_chunk(centres, min(chunk, N - s), args.noise, g)
        ids = torch.arange(s, s + x.shape[0], dtype=torch.int64, device="cuda")
        flat.add_with_ids(x, ids)
        pq.add_with_ids(x, ids)
        if Q is None:      # queries: perturbed rows of the set
            Q = torch.nn.functional.normalize(x[:256] + 0.05 * torch.nn.functional.normalize(torch.randn(256, d, generator=g, device="cuda"), dim=1), dim=1).contiguous()
    flat._finalize()
    pq._finalize()
    torch.cuda.synchronize()
    print(f"{N} x {d}, nlist {nlist}, m {m}: coarse k-means {t_coarse:.1f} s, codebooks {t_pq:.1f} s, all {time.time() - t0:.1f} s", flush=True)
    flat_bytes = flat._lists.nbytes() + flat.centroids.numel() * flat.centroids.element_size()
    res = {"rows": N, "dim": d, "nlist": nlist, "m": m, "k": k, "iters": args.iters, "device": torch.cuda.get_device_name(0),
           "train_seconds": {"coarse_kmeans": t_coarse, "codebooks": t_pq},
           "hbm_bytes": {"IndexIVFFlat": flat_bytes, f"IndexIVFPQ{m}": pq.hbm_bytes()}, "points": []}
    exact = FlatIPIndex(d).adopt(flat._lists.data, flat._lists.ids, id_base=0)
    _, If = exact.search_device(Q, k)
    If = If.cpu().numpy()
    for nprobe in (32, 1024):
        flat.nprobe = pq.nprobe = nprobe
        rec = {}
        for name, idx in (("IndexIVFFlat", flat), (f"IndexIVFPQ{m}", pq)):
            rec[name] = recall(idx.search_device(Q, k)[1].cpu().numpy(), If)
        for nq in (1, 256):
            q = Q[:nq].contiguous()
            point = {"nprobe": nprobe, "nq": nq}
            for name, idx in (("IndexIVFFlat", flat), (f"IndexIVFPQ{m}", pq)):
                t = timed(lambda: idx.search_device(q, k), args.iters)
                point[name] = {"seconds_per_search": t, "queries_per_s": nq / t, "recall_at_10": rec[name]}
            print(json.dumps(point), flush=True)
            res["points"].append(point)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"out": args.out, "hbm_bytes": res["hbm_bytes"]}))


if __name__ == "__main__":
    main()

"""Rank 0 of 8 of an IndexIVFFlat sharded across GPUs, emulated on one GPU.

A synthetic list-major index at the reference's evaluation shape (docs/Search-Index-Evaluation.md:110: 55M x 768,
nlist 74160; unit rows, list sizes drawn at random, centroids = normalised sample rows, no training), and rank 0's slice
of it: rows shard_range(N, 0, 8), a view of the first N/8 rows, with list_off clipped to it.  The probes come from the
coarse stage over the full centroid table (replicated on every rank, so it is timed once, apart).  Then the list scan
is timed three ways on the same probes:
  local    wise_ivf_scan_local_f32 over the slice (empty local segments compacted away)
  plain    wise_ivf_scan_f32 over the same clipped slice (every probe is a scan block and a merged list)
  whole    wise_ivf_scan_f32 over the whole index on one GPU
Settings: nprobe 1024 / k 1000 (the evaluations, docs/Retrieval-Evaluation.md:45) and nprobe 32 / k 20 (the REST
defaults, api/routes.py:902), at nq = 1 and nq = 256 (one batch of batched_text_search).  The merge of the 8 ranks'
answers and the all-gather are not in these figures (RCCL at world > 1 needs more than one GPU).

    python tools/ivf_shard_bench.py [--rows 55000000] [--iters 10] [--variants local,plain,whole] [--out FILE]
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
from wise_amd.index.ivf_flat import IVFFlatIPIndex  # noqa: E402
from wise_amd.index.sharded import shard_range  # noqa: E402


def make_index(N, d, nlist, seed=0, chunk=1 << 20):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.empty(N, d, dtype=torch.float32, device="cuda")
    for s in range(0, N, chunk):
        x = torch.randn(min(chunk, N - s), d, generator=g, device="cuda")
        X[s:s + x.shape[0]] = x / x.norm(dim=1, keepdim=True)
    sizes = np.random.default_rng(seed).multinomial(N, np.full(nlist, 1.0 / nlist))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ids = torch.arange(N, dtype=torch.int64, device="cuda") + 1
    pick = torch.from_numpy(np.random.default_rng(seed + 1).choice(N, nlist, replace=False)).cuda()
    c = X[pick].clone()
    return X, ids, off, c


def scan(lib, local, X, N, ids, off_d, nlist, Q, probes, k, D, I, ws, cnt=None):
    nq, nprobe = probes.shape
    if local:
        rc = lib.wise_ivf_scan_local_f32(X.data_ptr(), N, X.shape[1], off_d.data_ptr(), nlist, ids.data_ptr(), Q.data_ptr(),
                                         nq, probes.data_ptr(), nprobe, k, D.data_ptr(), I.data_ptr(), _lib.ptr(cnt),
                                         ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    else:
        rc = lib.wise_ivf_scan_f32(X.data_ptr(), N, X.shape[1], off_d.data_ptr(), nlist, ids.data_ptr(), Q.data_ptr(), nq,
                                   probes.data_ptr(), nprobe, k, D.data_ptr(), I.data_ptr(), ws.data_ptr(), ws.numel(),
                                   _lib.stream_ptr())
    _lib.check(rc, "scan")


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=55_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=74160)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--variants", default="local,plain,whole", help="which of the three scans to time")
    ap.add_argument("--out", default="ivf_shard_bench.json")
    args = ap.parse_args()
    lib = _lib.lib()
    N, d, nlist, W = args.rows, args.dim, args.nlist, args.world
    t0 = time.time()
    X, ids, off, c = make_index(N, d, nlist)
    torch.cuda.synchronize()
    print(f"index {N} x {d}, nlist {nlist}: built in {time.time() - t0:.1f} s", flush=True)
    lo, hi = shard_range(N, 0, W)
    loff = np.clip(off - lo, 0, hi - lo)
    off_d, loff_d = torch.from_numpy(off).cuda(), torch.from_numpy(loff).cuda()
    Xs, ids_s = X[lo:hi], ids[lo:hi]
    coarse = IVFFlatIPIndex(d, nlist)
    coarse.set_centroids(c)
    qg = torch.Generator(device="cuda").manual_seed(7)
    res = {"rows": N, "dim": d, "nlist": nlist, "world": W, "rank": 0, "slice_rows": hi - lo,
           "lists_held": int((np.diff(loff) > 0).sum()), "iters": args.iters, "settings": []}
    for nprobe, k in ((1024, 1000), (32, 20)):
        for nq in (1, 256):
            Q = torch.randn(nq, d, generator=qg, device="cuda")
            Q = (Q / Q.norm(dim=1, keepdim=True)).contiguous()
            probes = coarse.probes_device(Q, nprobe).contiguous()
            t_coarse = timed(lambda: coarse.probes_device(Q, nprobe), args.iters)
            D = torch.empty(nq, k, dtype=torch.float32, device="cuda")
            I = torch.empty(nq, k, dtype=torch.int64, device="cuda")
            cnt = torch.empty(nq, dtype=torch.int32, device="cuda")
            ws = torch.empty(max(lib.wise_ivf_scan_local_workspace_bytes(nq, nprobe, k),
                                 lib.wise_ivf_scan_workspace_bytes(nq, nprobe, k)), dtype=torch.uint8, device="cuda")
            runs = {
                "local": lambda: scan(lib, True, Xs, hi - lo, ids_s, loff_d, nlist, Q, probes, k, D, I, ws, cnt),
                "plain": lambda: scan(lib, False, Xs, hi - lo, ids_s, loff_d, nlist, Q, probes, k, D, I, ws),
                "whole": lambda: scan(lib, False, X, N, ids, off_d, nlist, Q, probes, k, D, I, ws),
            }
            # the two slice forms answer the same
            runs["local"]()
            Dl, Il = D.clone(), I.clone()
            runs["plain"]()
            same = bool(torch.equal(Dl.view(torch.int32), D.view(torch.int32)) and torch.equal(Il, I))
            row = {"nq": nq, "nprobe": nprobe, "k": k, "coarse_s": t_coarse, "slice_same_bits": same,
                   "probes_kept_mean": float(cnt.float().mean().item())}
            names = [v for v in ("local", "plain", "whole") if v in args.variants.split(",")]
            for name in names + names:                  # interleaved, the second round kept
                row[f"{name}_s"] = timed(runs[name], args.iters)
            for name in names:
                row[f"{name}_qps"] = nq / row[f"{name}_s"]
            if "local" in names and "plain" in names:
                row["local_vs_plain"] = row["plain_s"] / row["local_s"]
            print(json.dumps(row), flush=True)
            res["settings"].append(row)
            del ws
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

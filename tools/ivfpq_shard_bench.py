"""What one rank of an IndexIVFPQ<m> / IndexIVFPQ<m>R8 / R16 sharded over W GPUs does per search, measured on ONE GPU
(DESIGN.md §4), as tools/ivf_shard_bench.py does it for IndexIVFFlat: the index of tools/ivfpq_bench.py (same recipe, same
queries) is built whole, cut for W ranks by shard_range, and ONE rank's slice is timed.  Probes, bias and tables are computed
once per point (they are the same on every rank and not what sharding changes); timed, in seconds per call:
  a_whole_scan        wise_ivfpq_scan over the whole index                                  (one GPU holds everything)
  b_clipped_scan      wise_ivfpq_scan over the slice with list_off clipped to it            (what clipping offsets alone gives);
                      run `--repeats` times: b_clipped_scan is their median, b_spread = (max - min) / median
  c_local_scan        wise_ivfpq_scan_local over the slice
  at kc (the R types): a_whole_scan_kc, c_local_scan_kc (phase 1: the candidates), refine_whole_r8 / r16 (wise_ivf_refine over
  the whole store) and refine_local_r8 / r16 (phase 2: wise_ivf_refine_local over the slice, the global candidates of which
  about 1 / W lie in it)
and the ratios c / b (must not exceed 1 beyond b_spread) and c / (a / W).  The exchange (two all-gathers for the R types) is
NOT in these numbers: it needs more than one rank.

    timeout 1100 python tools/ivfpq_shard_bench.py [--rows 10000000] [--dim 512] [--m 64] [--world 8] [--rank 3] [--out FILE]

One GPU process: run it under a time limit of its own, as above.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from ivfpq_bench import rows_chunk, timed  # noqa: E402
from wise_amd import _lib  # noqa: E402
from wise_amd.index.ivf_flat import reference_nlist  # noqa: E402
from wise_amd.index.ivf_pq import KSUB, IVFPQRefineIPIndex  # noqa: E402
from wise_amd.index.sharded import shard_range  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--rank", type=int, default=3)
    ap.add_argument("--kc", type=int, default=500)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--noise", type=float, default=0.35)
    ap.add_argument("--out", default="ivfpq_shard_bench.json")
    args = ap.parse_args()
    N, d, m, k, W, kc = args.rows, args.dim, args.m, 10, args.world, args.kc
    nlist = reference_nlist(N)
    lib = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(0)
    centres = torch.nn.functional.normalize(torch.randn(max(nlist // 2, 16), d, generator=g, device="cuda"), dim=1)
    t0 = time.time()
    r8, r16 = IVFPQRefineIPIndex(d, nlist, m, 8), IVFPQRefineIPIndex(d, nlist, m, 16)
    train = rows_chunk(centres, min(N, 100 * nlist), args.noise, g)
    r8.train(train)
    r16.set_centroids(r8.centroids)
    r16.codebooks = r8.codebooks
    del train
    g = torch.Generator(device="cuda").manual_seed(1)
    Q, chunk = None, 1 << 20
    for s in range(0, N, chunk):
        x = rows_chunk(centres, min(chunk, N - s), args.noise, g)
        ids = torch.arange(s, s + x.shape[0], dtype=torch.int64, device="cuda")
        r8.add_with_ids(x, ids)
        r16.add_with_ids(x, ids)
        print(f"  added {s + x.shape[0]} rows, {time.time() - t0:.1f} s", flush=True)
        if Q is None:      # queries: perturbed rows of the set
            Q = torch.nn.functional.normalize(x[:256] + 0.05 * torch.nn.functional.normalize(torch.randn(256, d, generator=g, device="cuda"), dim=1), dim=1).contiguous()
    r8._finalize()
    r16._finalize()
    torch.cuda.synchronize()
    print(f"{N} x {d}, nlist {nlist}, m {m}: built in {time.time() - t0:.1f} s", flush=True)
    ls = r8._lists
    lo, hi = shard_range(N, args.rank, W)
    codes_s = ls.data[lo:hi].clone()                     # a rank's own allocation
    ids_s = ls.ids[lo:hi].clone()
    off_s = (ls.list_off - lo).clamp_(0, hi - lo).contiguous()
    stores = {}
    for idx in (r8, r16):
        rows, scales = idx._lists.extra[0], (idx._lists.extra[1] if idx.kind == 8 else None)
        stores[idx.kind] = (rows, scales, rows[lo:hi].clone(), None if scales is None else scales[lo:hi].clone())
    res = {"rows": N, "dim": d, "nlist": nlist, "m": m, "k": k, "kc": kc, "world": W, "rank": args.rank, "slice": [lo, hi],
           "iters": args.iters, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "points": []}
    st = _lib.stream_ptr()

    def scan(codes, n, off, ids, tabs, kk, D, I, local):
        lut, probes, bias, nq, nprobe = tabs
        fn = lib.wise_ivfpq_scan_local_workspace_bytes if local else lib.wise_ivfpq_scan_workspace_bytes
        ws = r8._workspace(fn(nq, nprobe, kk, m))
        head = (codes.data_ptr(), n, m, off.data_ptr(), nlist, _lib.ptr(ids), lut.data_ptr(), nq, probes.data_ptr(), bias.data_ptr(), nprobe, kk)
        if local:
            _lib.check(lib.wise_ivfpq_scan_local(*head, lo, D.data_ptr(), I.data_ptr(), 0, ws.data_ptr(), ws.numel(), st), "wise_ivfpq_scan_local")
        else:
            _lib.check(lib.wise_ivfpq_scan(*head, D.data_ptr(), I.data_ptr(), ws.data_ptr(), ws.numel(), st), "wise_ivfpq_scan")

    for nprobe in (32, 1024):
        for nq in (1, 256):
            q = Q[:nq].contiguous()
            probes = r8.probes_device(q, nprobe).contiguous()
            bias = torch.empty(nq, nprobe, dtype=torch.float32, device="cuda")
            _lib.check(lib.wise_pq_bias(q.data_ptr(), r8.centroids.data_ptr(), probes.data_ptr(), nq, nprobe, nlist, d, bias.data_ptr(), st), "wise_pq_bias")
            lut = torch.empty(nq, m, KSUB, dtype=torch.float32, device="cuda")
            _lib.check(lib.wise_pq_lut(q.data_ptr(), r8.codebooks.data_ptr(), nq, d, m, lut.data_ptr(), st), "wise_pq_lut")
            tabs = (lut, probes, bias, nq, nprobe)
            D, I = torch.empty(nq, k, device="cuda"), torch.empty(nq, k, dtype=torch.int64, device="cuda")
            cD, cand = torch.empty(nq, kc, device="cuda"), torch.empty(nq, kc, dtype=torch.int64, device="cuda")
            kept = ((off_s[1:] > off_s[:-1])[probes.clamp(min=0)] & (probes >= 0)).sum(dim=1).float().mean().item()
            p = {"nprobe": nprobe, "nq": nq, "kept_probes_mean": kept}
            p["a_whole_scan"] = timed(lambda: scan(ls.data, N, ls.list_off, ls.ids, tabs, k, D, I, False), args.iters)
            b, c = [], []
            for _ in range(args.repeats):                # interleaved: both see the same drift
                b.append(timed(lambda: scan(codes_s, hi - lo, off_s, ids_s, tabs, k, D, I, False), args.iters))
                c.append(timed(lambda: scan(codes_s, hi - lo, off_s, ids_s, tabs, k, D, I, True), args.iters))
            p["b_clipped_scan"], p["c_local_scan"] = statistics.median(b), statistics.median(c)
            p["b_spread"] = (max(b) - min(b)) / p["b_clipped_scan"]
            p["c_spread"] = (max(c) - min(c)) / p["c_local_scan"]
            p["c_over_b"] = p["c_local_scan"] / p["b_clipped_scan"]
            p["c_over_a_div_w"] = p["c_local_scan"] / (p["a_whole_scan"] / W)
            p["a_whole_scan_kc"] = timed(lambda: scan(ls.data, N, ls.list_off, None, tabs, kc, cD, cand, False), args.iters)
            p["c_local_scan_kc"] = timed(lambda: scan(codes_s, hi - lo, off_s, None, tabs, kc, cD, cand, True), args.iters)
            scan(ls.data, N, ls.list_off, None, tabs, kc, cD, cand, False)       # the global candidates both refines take
            for kind, (rows, scales, rows_s, scales_s) in stores.items():
                p[f"refine_whole_r{kind}"] = timed(lambda: _lib.check(lib.wise_ivf_refine(
                    rows.data_ptr(), kind, _lib.ptr(scales), N, d, ls.ids.data_ptr(), q.data_ptr(), nq, cand.data_ptr(), kc, k,
                    D.data_ptr(), I.data_ptr(), st), "wise_ivf_refine"), args.iters)
                p[f"refine_local_r{kind}"] = timed(lambda: _lib.check(lib.wise_ivf_refine_local(
                    rows_s.data_ptr(), kind, _lib.ptr(scales_s), hi - lo, d, ids_s.data_ptr(), q.data_ptr(), nq, cand.data_ptr(), kc, k, lo,
                    D.data_ptr(), I.data_ptr(), st), "wise_ivf_refine_local"), args.iters)
            print(json.dumps(p), flush=True)
            res["points"].append(p)
    res["exchange"] = "not measured: needs more than one rank"
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"out": args.out, "c_over_b_max": max(p["c_over_b"] for p in res["points"])}))


if __name__ == "__main__":
    main()

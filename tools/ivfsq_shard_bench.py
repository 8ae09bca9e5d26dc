"""What one rank of an IndexIVFSQ8 sharded over W GPUs does per search, measured on ONE GPU, as tools/ivfpq_shard_bench.py does
it for IndexIVFPQ<m>: the IndexIVFSQ8 of tools/ivfsq_bench.py (same recipe, same queries) is built whole, cut for W ranks by
shard_range, and ONE rank's slice is timed.  Probes, bias and the weight rows are computed once per point (they are the same on
every rank and not what sharding changes); timed, in seconds per call, at nprobe 32 and 1024 and nq 1 and 256:
  a_whole_scan        wise_ivfsq_scan over the whole index                                  (one GPU holds everything)
  b_clipped_scan      wise_ivfsq_scan over the slice with list_off clipped to it            (what clipping offsets alone gives);
                      run `--repeats` times: b_clipped_scan is their median, b_spread = (max - min) / median
  c_local_scan        wise_ivfsq_scan_local over the slice
and the ratios c / b and c / (a / W), the per-rank HBM bytes beside the whole index's, and — once, at the first point — whether
the W slices' answers merged in rank order have the bits of the whole scan.  The exchange is NOT in these numbers: it needs more
than one rank.

    timeout 1100 python tools/ivfsq_shard_bench.py [--rows 10000000] [--dim 512] [--world 8] [--rank 3] [--out FILE]

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
from ivfsq_bench import chunk, timed  # noqa: E402
from wise_amd import _lib  # noqa: E402
from wise_amd.index.ivf_flat import reference_nlist  # noqa: E402
from wise_amd.index.ivf_sq import IVFSQIPIndex  # noqa: E402
from wise_amd.index.sharded import merge_device, shard_range  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--rank", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--noise", type=float, default=0.35)
    ap.add_argument("--out", default="profiles/ivfsq_shard_bench.json")
    args = ap.parse_args()
    N, d, k, W = args.rows, args.dim, 10, args.world
    nlist = reference_nlist(N)
    lib = _lib.lib()
    t0 = time.time()
    g = torch.Generator(device="cuda").manual_seed(0)
    centres = torch.nn.functional.normalize(torch.randn(max(nlist // 2, 16), d, generator=g, device="cuda"), dim=1)
    g = torch.Generator(device="cuda").manual_seed(1)
    train = chunk(centres, args.noise, min(N, 100 * nlist), g)
    sq8 = IVFSQIPIndex(d, nlist)
    sq8.train(train)
    del train
    g = torch.Generator(device="cuda").manual_seed(2)
    Q = None
    for s in range(0, N, 1 << 20):
        x = chunk(centres, args.noise, min(1 << 20, N - s), g)
        sq8.add_with_ids(x, torch.arange(s, s + x.shape[0], dtype=torch.int64, device="cuda"))
        if Q is None:      # queries: perturbed rows of the set
            Q = torch.nn.functional.normalize(x[:256] + 0.05 * torch.nn.functional.normalize(torch.randn(256, d, generator=g, device="cuda"), dim=1), dim=1).contiguous()
    sq8._finalize()
    torch.cuda.synchronize()
    print(f"{N} x {d}, nlist {nlist}: built in {time.time() - t0:.1f} s", flush=True)
    ls = sq8._lists

    def cut(r):
        a, b = shard_range(N, r, W)
        return a, b, ls.data[a:b].clone(), ls.ids[a:b].clone(), (ls.list_off - a).clamp_(0, b - a).contiguous()    # a rank's own allocations

    lo, hi, codes_s, ids_s, off_s = cut(args.rank)
    mine = IVFSQIPIndex(d, nlist)
    mine.set_centroids(sq8.centroids)
    mine.trained = sq8.trained
    mine.adopt_lists(codes_s, ids_s, off_s, pos_base=lo)
    res = {"rows": N, "dim": d, "nlist": nlist, "k": k, "world": W, "rank": args.rank, "slice": [lo, hi], "iters": args.iters,
           "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
           "hbm_bytes": {"whole_index": sq8.hbm_bytes(), "one_rank": mine.hbm_bytes()}, "points": []}
    st = _lib.stream_ptr()

    def scan(codes, n, off, ids, tabs, D, I, local, pos_base=0):
        Wq, q0, probes, bias, nq, nprobe = tabs
        fn = lib.wise_ivfsq_scan_local_workspace_bytes if local else lib.wise_ivfsq_scan_workspace_bytes
        ws = sq8._workspace(fn(nq, nprobe, k))
        head = (codes.data_ptr(), n, d, off.data_ptr(), nlist, _lib.ptr(ids), Wq.data_ptr(), q0.data_ptr(), nq, probes.data_ptr(),
                bias.data_ptr(), nprobe, k)
        if local:
            _lib.check(lib.wise_ivfsq_scan_local(*head, pos_base, D.data_ptr(), I.data_ptr(), 0, ws.data_ptr(), ws.numel(), st),
                       "wise_ivfsq_scan_local")
        else:
            _lib.check(lib.wise_ivfsq_scan(*head, D.data_ptr(), I.data_ptr(), ws.data_ptr(), ws.numel(), st), "wise_ivfsq_scan")

    for nprobe in (32, 1024):
        for nq in (1, 256):
            q = Q[:nq].contiguous()
            probes = sq8.probes_device(q, nprobe).contiguous()
            bias = torch.empty(nq, nprobe, dtype=torch.float32, device="cuda")
            _lib.check(lib.wise_pq_bias(q.data_ptr(), sq8.centroids.data_ptr(), probes.data_ptr(), nq, nprobe, nlist, d, bias.data_ptr(), st), "wise_pq_bias")
            Wq, q0 = torch.empty(nq, d, dtype=torch.float32, device="cuda"), torch.empty(nq, dtype=torch.float32, device="cuda")
            _lib.check(lib.wise_sq_query(q.data_ptr(), sq8.trained.data_ptr(), nq, d, Wq.data_ptr(), q0.data_ptr(), st), "wise_sq_query")
            tabs = (Wq, q0, probes, bias, nq, nprobe)
            D, I = torch.empty(nq, k, device="cuda"), torch.empty(nq, k, dtype=torch.int64, device="cuda")
            kept = ((off_s[1:] > off_s[:-1])[probes.clamp(min=0)] & (probes >= 0)).sum(dim=1).float().mean().item()
            p = {"nprobe": nprobe, "nq": nq, "kept_probes_mean": kept}
            if not res["points"]:                        # once: the W slices merged in rank order against the whole scan
                scan(ls.data, N, ls.list_off, ls.ids, tabs, D, I, False)
                Ds, Is = [], []
                for r in range(W):
                    a, b, c_r, i_r, o_r = cut(r)
                    Dr, Ir = torch.empty_like(D), torch.empty_like(I)
                    scan(c_r, b - a, o_r, i_r, tabs, Dr, Ir, True, a)
                    Ds.append(Dr)
                    Is.append(Ir)
                Dm, Im = merge_device(torch.stack(Ds), torch.stack(Is), k)
                res["merged_slices_equal_whole_scan"] = bool(torch.equal(Dm.view(torch.int32), D.view(torch.int32)) and torch.equal(Im, I))
                del Ds, Is
            p["a_whole_scan"] = timed(lambda: scan(ls.data, N, ls.list_off, ls.ids, tabs, D, I, False), args.iters)
            b, c = [], []
            for _ in range(args.repeats):                # interleaved: both see the same drift
                b.append(timed(lambda: scan(codes_s, hi - lo, off_s, ids_s, tabs, D, I, False), args.iters))
                c.append(timed(lambda: scan(codes_s, hi - lo, off_s, ids_s, tabs, D, I, True, lo), args.iters))
            p["b_clipped_scan"], p["c_local_scan"] = statistics.median(b), statistics.median(c)
            p["b_spread"] = (max(b) - min(b)) / p["b_clipped_scan"]
            p["c_spread"] = (max(c) - min(c)) / p["c_local_scan"]
            p["c_over_b"] = p["c_local_scan"] / p["b_clipped_scan"]
            p["c_over_a_div_w"] = p["c_local_scan"] / (p["a_whole_scan"] / W)
            print(json.dumps(p), flush=True)
            res["points"].append(p)
    res["exchange"] = "not measured: needs more than one rank"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"out": args.out, "c_over_b_max": max(p["c_over_b"] for p in res["points"]),
                      "merged_slices_equal_whole_scan": res["merged_slices_equal_whole_scan"]}))


if __name__ == "__main__":
    main()

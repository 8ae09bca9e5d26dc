"""IndexIVFPQ<m>R8 / IndexIVFPQ<m>R16 beside IndexIVFPQ<m> and IndexIVFFlat on the same rows, the same coarse quantizer, the same
codebooks, the same box, the same run: what re-ranking buys per byte and what it costs.

The data recipe, the queries and the timing are tools/ivfpq_bench.py's.  The two re-ranking indexes take the IndexIVFFlat's
centroids and one set of codebooks; the plain IndexIVFPQ<m> adopts the R8 index's codes (the same tensors: no copy).  Reported:
  hbm_bytes        of the four indexes
  points           seconds per `search_device`, queries/s and recall@10 against the exhaustive answer at nq in {1, 256},
                   nprobe in {32, 1024}, k = 10 — the re-ranking indexes at the chosen k_factor
  k_factor_sweep   recall@10 and seconds per search (nq = 256) for k_factor in {1, 2, 5, 10, 20, 50, 100, 200}, both stores,
                   both nprobe; chosen = the smallest k_factor whose recall is within 0.01 of the largest one's, worst case over
                   stores and nprobe — the number wise_amd/index/ivf_pq.py DEFAULT_K_FACTOR cites
  stages           at the chosen k_factor: the coarse stage + tables + PQ scan at k and at kc = k * k_factor (their difference
                   is the extra scan time re-ranking asks for) and wise_ivf_refine alone, in seconds per call

    timeout 1100 python tools/ivfpq_refine_bench.py [--rows 10000000] [--dim 512] [--m 64] [--iters 10] [--out FILE]

One GPU process: run it under a time limit of its own, as above.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from ivfpq_bench import recall, rows_chunk, timed  # noqa: E402
from wise_amd import _lib  # noqa: E402
from wise_amd.index.flat_ip import FlatIPIndex  # noqa: E402
from wise_amd.index.ivf_flat import IVFFlatIPIndex, reference_nlist  # noqa: E402
from wise_amd.index.ivf_pq import IVFPQIPIndex, IVFPQRefineIPIndex  # noqa: E402

K_FACTORS = (1, 2, 5, 10, 20, 50, 100, 200)


def choose_k_factor(sweep):
    """The smallest k_factor whose recall is within 0.01 of the largest k_factor's, in every (store, nprobe) series."""
    chosen = K_FACTORS[0]
    for series in sweep.values():
        top = series[str(K_FACTORS[-1])]["recall_at_10"]
        chosen = max(chosen, next(f for f in K_FACTORS if series[str(f)]["recall_at_10"] >= top - 0.01))
    return chosen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--noise", type=float, default=0.35)
    ap.add_argument("--out", default="ivfpq_refine_bench.json")
    args = ap.parse_args()
    N, d, m, k = args.rows, args.dim, args.m, 10
    nlist = reference_nlist(N)
    g = torch.Generator(device="cuda").manual_seed(0)
    centres = torch.nn.functional.normalize(torch.randn(max(nlist // 2, 16), d, generator=g, device="cuda"), dim=1)
    chunk = 1 << 20
    t0 = time.time()
    flat, pq = IVFFlatIPIndex(d, nlist), IVFPQIPIndex(d, nlist, m)
    r8, r16 = IVFPQRefineIPIndex(d, nlist, m, 8), IVFPQRefineIPIndex(d, nlist, m, 16)
    train = rows_chunk(centres, min(N, 100 * nlist), args.noise, g)
    flat.train(train)
    for idx in (pq, r8, r16):
        idx.set_centroids(flat.centroids)
    r8.codebooks = r16.codebooks = pq.codebooks = r8.train_codebooks(r8.training_residuals(train))
    del train
    g = torch.Generator(device="cuda").manual_seed(1)
    Q = None
    for s in range(0, N, chunk):
        x = rows_chunk(centres, min(chunk, N - s), args.noise, g)
        ids = torch.arange(s, s + x.shape[0], dtype=torch.int64, device="cuda")
        for idx in (flat, r8, r16):
            idx.add_with_ids(x, ids)
        print(f"  added {s + x.shape[0]} rows, {time.time() - t0:.1f} s", flush=True)
        if Q is None:      # queries: perturbed rows of the set
            Q = torch.nn.functional.normalize(x[:256] + 0.05 * torch.nn.functional.normalize(torch.randn(256, d, generator=g, device="cuda"), dim=1), dim=1).contiguous()
    for idx in (flat, r8, r16):
        idx._finalize()
    pq.adopt_lists(r8._lists.data, r8._lists.ids, r8._lists.list_off)
    torch.cuda.synchronize()
    print(f"{N} x {d}, nlist {nlist}, m {m}: built in {time.time() - t0:.1f} s", flush=True)
    names = {"IndexIVFFlat": flat, f"IndexIVFPQ{m}": pq, f"IndexIVFPQ{m}R8": r8, f"IndexIVFPQ{m}R16": r16}
    flat_bytes = flat._lists.nbytes() + flat.centroids.numel() * flat.centroids.element_size()
    res = {"rows": N, "dim": d, "nlist": nlist, "m": m, "k": k, "iters": args.iters, "device": torch.cuda.get_device_name(0),
           "hbm_bytes": {n: (flat_bytes if i is flat else i.hbm_bytes()) for n, i in names.items()},
           "k_factor_sweep": {}, "points": [], "stages": []}
    exact = FlatIPIndex(d).adopt(flat._lists.data, flat._lists.ids, id_base=0)
    If = exact.search_device(Q, k)[1].cpu().numpy()
    for nprobe in (32, 1024):
        for name in (f"IndexIVFPQ{m}R8", f"IndexIVFPQ{m}R16"):
            idx, series = names[name], {}
            idx.nprobe = nprobe
            for f in K_FACTORS:
                idx.k_factor = f
                series[str(f)] = {"candidates": idx.candidates(k), "recall_at_10": recall(idx.search_device(Q, k)[1].cpu().numpy(), If),
                                  "seconds_per_search_nq256": timed(lambda: idx.search_device(Q, k), max(args.iters // 2, 2))}
            print(json.dumps({"nprobe": nprobe, name: series}), flush=True)
            res["k_factor_sweep"][f"{name} nprobe {nprobe}"] = series
    chosen = res["chosen_k_factor"] = choose_k_factor(res["k_factor_sweep"])
    r8.k_factor = r16.k_factor = chosen
    for nprobe in (32, 1024):
        rec = {}
        for name, idx in names.items():
            idx.nprobe = nprobe
            rec[name] = recall(idx.search_device(Q, k)[1].cpu().numpy(), If)
        for nq in (1, 256):
            q = Q[:nq].contiguous()
            point = {"nprobe": nprobe, "nq": nq}
            for name, idx in names.items():
                t = timed(lambda: idx.search_device(q, k), args.iters)
                point[name] = {"seconds_per_search": t, "queries_per_s": nq / t, "recall_at_10": rec[name]}
            print(json.dumps(point), flush=True)
            res["points"].append(point)
            # the stages of the re-ranking search, each alone
            kc = r8.candidates(k)
            D, I = torch.empty(nq, k, device="cuda"), torch.empty(nq, k, dtype=torch.int64, device="cuda")
            cD, cand = torch.empty(nq, kc, device="cuda"), torch.empty(nq, kc, dtype=torch.int64, device="cuda")
            stage = {"nprobe": nprobe, "nq": nq, "k": k, "kc": kc,
                     "scan_at_k_seconds": timed(lambda: r8._scan(q, k, D, I, positions=True), args.iters),
                     "scan_at_kc_seconds": timed(lambda: r8._scan(q, kc, cD, cand, positions=True), args.iters)}
            lib = _lib.lib()
            for idx, key in ((r8, "refine_r8_seconds"), (r16, "refine_r16_seconds")):
                rows, scales = idx._store()
                stage[key] = timed(lambda: _lib.check(lib.wise_ivf_refine(
                    rows, idx.kind, scales, idx.ntotal, d, idx._lists.ids.data_ptr(), q.data_ptr(), nq, cand.data_ptr(), kc, k,
                    D.data_ptr(), I.data_ptr(), _lib.stream_ptr()), "wise_ivf_refine"), args.iters)
            print(json.dumps(stage), flush=True)
            res["stages"].append(stage)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({"out": args.out, "hbm_bytes": res["hbm_bytes"], "chosen_k_factor": chosen}))


if __name__ == "__main__":
    main()

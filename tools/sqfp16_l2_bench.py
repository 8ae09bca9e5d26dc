"""IndexSQfp16L2 beside IndexFlatL2 on the same rows, the same box, the same run (README.md).

One seeded clustered set of rows that are NOT normalised (unit directions around `--centres` clusters times lengths log-uniform over
[1, 4]) is generated on the device chunk by chunk; IndexFlatL2 adopts the fp32 tensor, IndexSQfp16L2 the same rows rounded to binary16
(the encoder's bits).  Timing: every shape is warmed up first (both indexes build what their batched searches keep then); then the
callables of a point ALTERNATE call by call — HIP events around the single call — for --iters rounds (at least 10), so that clock and
thermal drift fall on all alike; a point reports the median with the smallest and the largest call (the spread).

  per nq in 1, 3, 4, 8, 32, 256
      IndexSQfp16L2_exact     wise_l2sq16_topk: passes of up to 4 queries, N d 2 bytes a pass
      IndexSQfp16L2_batched   wise_l2sq16_topk_batched (nq >= 3): the matrix-core passes over the same binary16 rows
      IndexFlatL2             search_device as its class routes it (the exact scan under 8 queries, its bf16 passes from 8)
  crossover    the smallest measured batch from which IndexSQfp16L2's batched search beats its exact scan at every larger measured
               one: what FlatSQfp16L2Index.BATCH_MIN_QUERIES should be
  recall       recall@k of IndexSQfp16L2 against IndexFlatL2 over the 256 queries; HBM bytes; who answered the batched queries

There is no pass mark.

    timeout 1100 python tools/sqfp16_l2_bench.py [--rows 10000000] [--dim 512] [--out profiles/sqfp16_l2_bench.json]

One GPU process: run it under a time limit of its own, as above.  At 10M x 512 the fp32 rows are 20.5 GB, IndexFlatL2's bf16 copy
and half-norms 10.3 GB, the binary16 rows 10.2 GB and their half-norms 40 MB.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from flatl2_bench import alternate, chunk, show  # noqa: E402
from wise_amd import _lib  # noqa: E402
from wise_amd.index.flat_l2 import FlatL2Index  # noqa: E402
from wise_amd.index.flat_sq import FlatSQfp16L2Index  # noqa: E402

NQS = (1, 3, 4, 8, 32, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--centres", type=int, default=4096)
    ap.add_argument("--noise", type=float, default=0.35)
    ap.add_argument("--spread", type=float, default=4.0)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "sqfp16_l2_bench.json"))
    a = ap.parse_args()
    if a.iters < 10:
        ap.error("--iters must be at least 10")
    N, d, k = a.rows, a.dim, a.k
    lib = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(1)
    centres = torch.nn.functional.normalize(torch.randn(a.centres, d, generator=g, device="cuda"), dim=1)
    t0 = time.time()
    X = torch.empty(N, d, dtype=torch.float32, device="cuda")
    H = torch.empty(N, d, dtype=torch.float16, device="cuda")
    step = 1 << 19
    for s in range(0, N, step):
        n = min(step, N - s)
        length = torch.exp(torch.rand(n, 1, generator=g, device="cuda") * math.log(a.spread))
        X[s:s + n] = chunk(centres, a.noise, n, g) * length
        H[s:s + n] = X[s:s + n].half()                # round to nearest even, subnormals kept: wise_sq16_encode's bits
    ids = torch.arange(N, device="cuda", dtype=torch.int64)
    l2 = FlatL2Index(d).adopt(X, ids)
    sq = FlatSQfp16L2Index(d).adopt(H, ids)
    torch.cuda.synchronize()
    gq = torch.Generator(device="cuda").manual_seed(2)
    rows = torch.randint(0, N, (max(NQS),), generator=gq, device="cuda")
    Q = (X[rows] * (1.0 + 0.05 * torch.randn(max(NQS), d, generator=gq, device="cuda"))).contiguous()
    out = {"what": "tools/sqfp16_l2_bench.py: IndexSQfp16L2 (binary16 rows) and IndexFlatL2 (the same rows in fp32) alternating call by call "
                   "in one run; seconds are of one call (median, min, max of `calls` timed calls after warm-up)",
           "rows": N, "dim": d, "k": k, "iters": a.iters, "centres": a.centres, "noise": a.noise, "spread": a.spread,
           "build_seconds": time.time() - t0, "device": torch.cuda.get_device_name(0),
           "provisional_batch_min_rows": sq.BATCH_MIN_ROWS, "provisional_batch_min_queries": sq.BATCH_MIN_QUERIES, "points": {}}

    _, Il2 = l2.search_device(Q, k)
    _, Isq = sq.search_device(Q, k)
    out["recall_at_k_against_IndexFlatL2"] = float(((Il2.unsqueeze(2) == Isq.unsqueeze(1)).any(dim=2).float().sum(dim=1) / k).mean())

    def exact(q, D, I, ws):
        def run():
            _lib.check(lib.wise_l2sq16_topk(H.data_ptr(), N, d, q.data_ptr(), q.shape[0], k, ids.data_ptr(), 0, D.data_ptr(), I.data_ptr(),
                                            ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "wise_l2sq16_topk")
        return run

    sq.BATCH_MIN_QUERIES = 3                        # from here on search_device of IndexSQfp16L2 IS the batched search where it is served
    wins = {}
    for nq in NQS:
        q = Q[:nq].contiguous()
        D = torch.empty(nq, k, dtype=torch.float32, device="cuda")
        I = torch.empty(nq, k, dtype=torch.int64, device="cuda")
        ws = torch.empty(lib.wise_l2sqfp16_topk_workspace_bytes(N, d, nq, k), dtype=torch.uint8, device="cuda")
        fns = {"IndexSQfp16L2_exact": exact(q, D, I, ws)}
        if nq >= 3:
            fns["IndexSQfp16L2_batched"] = lambda: sq.search_device(q, k)
        fns["IndexFlatL2"] = lambda: l2.search_device(q, k)
        res = alternate(fns, a.iters)
        for r in res.values():
            r["queries_per_second"] = nq / r["median"]
        res["IndexSQfp16L2_exact"]["bytes_per_pass"] = N * d * 2
        best = min(r["median"] for n_, r in res.items() if n_.startswith("IndexSQfp16L2"))
        res["ratio_sqfp16l2_exact_to_flatl2"] = res["IndexSQfp16L2_exact"]["median"] / res["IndexFlatL2"]["median"]
        res["ratio_sqfp16l2_best_to_flatl2"] = best / res["IndexFlatL2"]["median"]
        out["points"][f"nq{nq}"] = res
        show(f"nq={nq}", {n_: r for n_, r in res.items() if isinstance(r, dict)})
        if nq >= 3:
            wins[nq] = res["IndexSQfp16L2_batched"]["median"] < res["IndexSQfp16L2_exact"]["median"]
    out["batched_wins_at"] = {str(nq): w for nq, w in wins.items()}
    out["measured_crossover_batch_size"] = next((nq for nq in wins if all(wins[m] for m in wins if m >= nq)), None)
    out["single_query_ratio_to_IndexFlatL2"] = out["points"]["nq1"]["ratio_sqfp16l2_exact_to_flatl2"]
    out["hbm_bytes"] = {"IndexSQfp16L2": {"rows_and_ids": sq.hbm_bytes(), "half_norms_and_norm": 0 if sq._half is None else N * 4 + 4},
                        "IndexFlatL2": {"rows_and_ids": l2.hbm_bytes(), "bf16_copy_and_half_norms": 0 if l2._Xb is None else N * (2 * d + 4)}}
    out["batched_counters"] = {"IndexSQfp16L2": dict(zip(("answered_from_lists", "handed_to_exact_scan"), sq.batched_counts())),
                               "IndexFlatL2": dict(zip(("answered_from_lists", "handed_to_exact_scan"), l2.batched_counts()))}
    print(json.dumps({k_: out[k_] for k_ in ("batched_wins_at", "measured_crossover_batch_size", "single_query_ratio_to_IndexFlatL2",
                                             "hbm_bytes", "batched_counters", "recall_at_k_against_IndexFlatL2")}), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

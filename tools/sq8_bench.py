"""IndexSQ8bit beside IndexSQfp16 and IndexFlatIP (default shadows) on the same rows, the same box, the same run (DESIGN.md §4,
README.md): bytes held, the time of one search call at nq = 1, 3, 4, 8, 16, 32 and 256, recall@10 against the fp32 answer, and the
batch size from which wise_ipsq8_topk_batched wins.

One seeded clustered set is generated on the device chunk by chunk (tools/sqfp16_bench.py's recipe).  IndexFlatIP adopts the fp32
tensor; IndexSQfp16 and IndexSQ8bit encode it on the GPU (IndexSQ8bit trains its ranges over every row first).  Timing: every shape
is warmed up first (IndexFlatIP builds its shadows then); then the callables of a point ALTERNATE call by call — HIP events around
the single call — for --iters rounds (at least 10), so that clock and thermal drift fall on all alike; a point reports the median
with the smallest and the largest call (the spread).

  search       every nq: search_device of the three indexes as their classes route it
  crossover    every nq >= 3: wise_ipsq8_topk_batched beside the exact scan's 4-query passes (wise_ipsq8_topk); the smallest measured
               batch from which the batched search wins at every larger measured one is what FlatSQ8IPIndex.BATCH_MIN_QUERIES should
               be (the rule IndexFlatL2 recorded)

There is no pass mark.

    timeout 1100 python tools/sq8_bench.py [--rows 10000000] [--dim 512] [--out profiles/sq8_bench.json]

One GPU process: run it under a time limit of its own, as above.  At 10M x 512 the fp32 rows are 20.5 GB and IndexFlatIP's shadows
15.4 GB; IndexSQfp16 holds 10.3 GB and IndexSQ8bit 5.2 GB.
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
from wise_amd import _lib  # noqa: E402
from wise_amd.index.flat_ip import FlatIPIndex  # noqa: E402
from wise_amd.index.flat_sq import FlatSQ8IPIndex, FlatSQfp16IPIndex  # noqa: E402

NQS = (1, 3, 4, 8, 16, 32, 256)


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


def alternate(fns: dict, iters: int, warmup: int = 3) -> dict:
    """name -> {median, min, max} seconds of one call, the callables taking turns round by round"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(iters):
        for name, fn in fns.items():
            times[name].append(one_call_seconds(fn))
    return {name: {"median": statistics.median(t), "min": min(t), "max": max(t), "calls": len(t)} for name, t in times.items()}


def show(tag, res):
    print(f"{tag}: " + ", ".join(f"{n} {r['median'] * 1e3:.3f} ms [{r['min'] * 1e3:.3f}, {r['max'] * 1e3:.3f}]" for n, r in res.items()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--centres", type=int, default=4096)
    ap.add_argument("--noise", type=float, default=0.35)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "sq8_bench.json"))
    a = ap.parse_args()
    if a.iters < 10:
        ap.error("--iters must be at least 10")
    N, d, k = a.rows, a.dim, a.k
    lib = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(1)
    centres = torch.nn.functional.normalize(torch.randn(a.centres, d, generator=g, device="cuda"), dim=1)
    t0 = time.time()
    X = torch.empty(N, d, dtype=torch.float32, device="cuda")
    step = 1 << 19
    for s in range(0, N, step):
        n = min(step, N - s)
        X[s:s + n] = chunk(centres, a.noise, n, g)
    ids = torch.arange(N, device="cuda", dtype=torch.int64)
    flat = FlatIPIndex(d).adopt(X, ids)        # default shadows: int8 for single queries, bf16 for the batched passes
    sq16 = FlatSQfp16IPIndex(d)
    sq16.reserve(N)
    sq8 = FlatSQ8IPIndex(d)
    sq8.train(X)                               # the ranges over every row, as create_index trains them
    sq8.reserve(N)
    for s in range(0, N, step):
        sq16.add_with_ids(X[s:s + step], ids[s:s + step])
        sq8.add_with_ids(X[s:s + step], ids[s:s + step])
    torch.cuda.synchronize()
    gq = torch.Generator(device="cuda").manual_seed(2)
    rows = torch.randint(0, N, (max(NQS),), generator=gq, device="cuda")
    Q = torch.nn.functional.normalize(X[rows] + 0.05 * torch.nn.functional.normalize(torch.randn(max(NQS), d, generator=gq, device="cuda"), dim=1),
                                      dim=1).contiguous()
    out = {"what": "tools/sq8_bench.py: IndexSQ8bit, IndexSQfp16 and IndexFlatIP (default shadows) alternating call by call in one run; "
                   "seconds are of one call (median, min, max of `calls` timed calls after warm-up)",
           "rows": N, "dim": d, "k": k, "iters": a.iters, "centres": a.centres, "noise": a.noise, "build_seconds": time.time() - t0,
           "device": torch.cuda.get_device_name(0), "batch_min_rows": sq8.BATCH_MIN_ROWS, "batch_min_queries": sq8.BATCH_MIN_QUERIES,
           "points": {}}

    # recall@k against the fp32 answer (the fp32 scan itself: shadows off for this call)
    exact = FlatIPIndex(d, shadow=False).adopt(flat._X, flat._ids)
    _, If = exact.search_device(Q, k)
    recall = {}
    for name, idx in (("IndexSQ8bit", sq8), ("IndexSQfp16", sq16), ("IndexFlatIP", flat)):
        _, I = idx.search_device(Q, k)
        recall[name] = float(((I.unsqueeze(2) == If.unsqueeze(1)).any(dim=2).float().sum(dim=1) / k).mean())
    out["recall_at_k_vs_fp32"] = recall
    del exact

    for nq in NQS:
        q = Q[:nq].contiguous()
        res = alternate({"IndexSQ8bit": lambda: sq8.search_device(q, k), "IndexSQfp16": lambda: sq16.search_device(q, k),
                         "IndexFlatIP": lambda: flat.search_device(q, k)}, a.iters)
        for r in res.values():
            r["queries_per_second"] = nq / r["median"]
        res["ratio_sq8_to_sqfp16"] = res["IndexSQ8bit"]["median"] / res["IndexSQfp16"]["median"]
        res["ratio_sq8_to_flat"] = res["IndexSQ8bit"]["median"] / res["IndexFlatIP"]["median"]
        out["points"][f"nq{nq}"] = res
        show(f"search nq={nq}", {n: r for n, r in res.items() if isinstance(r, dict)})
    res1 = out["points"]["nq1"]["IndexSQ8bit"]
    res1["bytes"] = N * d
    res1["bytes_per_second"] = N * d / res1["median"]

    # the crossover: the batched search beside the exact scan's 4-query passes
    C, T = sq8._codes_t, sq8._trained
    (norms,) = sq8._batch_operands()
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    wins = {}
    for nq in NQS[1:]:
        q = Q[:nq].contiguous()
        D = torch.empty(nq, k, dtype=torch.float32, device="cuda")
        I = torch.empty(nq, k, dtype=torch.int64, device="cuda")
        ws = torch.empty(lib.wise_ipsq8_topk_workspace_bytes(N, d, nq, k), dtype=torch.uint8, device="cuda")
        wb = torch.empty(lib.wise_ipsq8_topk_batched_workspace_bytes(N, d, nq, k), dtype=torch.uint8, device="cuda")

        def scan():
            _lib.check(lib.wise_ipsq8_topk(C.data_ptr(), T.data_ptr(), N, d, q.data_ptr(), nq, k, ids.data_ptr(), 0, D.data_ptr(), I.data_ptr(),
                                           ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "wise_ipsq8_topk")

        def batched():
            _lib.check(lib.wise_ipsq8_topk_batched(C.data_ptr(), T.data_ptr(), norms.data_ptr(), N, d, q.data_ptr(), nq, k, ids.data_ptr(), 0,
                                                   D.data_ptr(), I.data_ptr(), counters.data_ptr(), wb.data_ptr(), wb.numel(),
                                                   _lib.stream_ptr()), "wise_ipsq8_topk_batched")
        res = alternate({"batched": batched, "exact_scan_passes": scan}, a.iters)
        out["points"][f"small_batch_nq{nq}"] = res
        show(f"nq={nq}", res)
        wins[nq] = res["batched"]["median"] < res["exact_scan_passes"]["median"]
    out["batched_wins_at"] = {str(nq): w for nq, w in wins.items()}
    out["measured_crossover_batch_size"] = next((nq for nq in NQS[1:] if all(wins[m] for m in NQS[1:] if m >= nq)), None)
    c = counters.cpu()
    out["batched_counters"] = {"answered_from_lists": int(c[0]), "handed_to_exact_scan": int(c[1])}
    out["hbm_bytes"] = {"IndexSQ8bit": sq8.hbm_bytes(), "IndexSQfp16": sq16.hbm_bytes(),
                        "IndexFlatIP": {"rows_and_ids": N * (4 * d + 8), "int8_shadow": 0 if flat._Xq is None else N * (d + 4),
                                        "bf16_shadow": 0 if flat._Xb is None else N * d * 2}}
    fb = out["hbm_bytes"]["IndexFlatIP"]
    out["hbm_ratio_to_sqfp16"] = sq8.hbm_bytes() / sq16.hbm_bytes()
    out["hbm_ratio_to_flat"] = sq8.hbm_bytes() / (fb["rows_and_ids"] + fb["int8_shadow"] + fb["bf16_shadow"])
    print(json.dumps({k_: out[k_] for k_ in ("batched_wins_at", "measured_crossover_batch_size", "hbm_bytes", "hbm_ratio_to_sqfp16",
                                             "hbm_ratio_to_flat", "batched_counters", "recall_at_k_vs_fp32")}), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

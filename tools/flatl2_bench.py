"""IndexFlatL2 beside IndexFlatIP(shadow=False) on the same rows, the same box, the same run (README.md).

One seeded clustered set is generated on the device chunk by chunk (tools/sqfp16_bench.py's recipe) and BOTH indexes adopt the one
fp32 tensor: they read the same bytes.  Timing: every shape is warmed up first (IndexFlatL2 builds its bf16 copy and half-norms
then); then the callables of a point ALTERNATE call by call — HIP events around the single call — for --iters rounds (at least 10),
so that clock and thermal drift fall on all alike; a point reports the median with the smallest and the largest call (the spread).

  search       nq = 1, 8, 32, 256: search_device of the two indexes as their classes route it
  exact scan   wise_l2_topk_f32 beside wise_ip_topk_f32 at one and at four queries a pass: the two read exactly the same bytes, so
               the ratio of their times per pass is the cost of a subtraction per element
  batched      wise_l2_topk_batched at nq = 256 beside IndexFlatIP's bf16 batched pass (a third index, shadow="bf16", over the same
               rows): both read a bf16 copy of the rows on the matrix cores
  crossover    nq = 3, 4, 8, 12, 16, 32: the batched search beside the exact scan's 4-query passes; the smallest measured batch from
               which the batched search wins at every larger measured size is what FlatL2Index.BATCH_MIN_QUERIES should be (a
               whole pass of 4 can win where 3 queries, two passes, lose)

There is no pass mark.

    timeout 1100 python tools/flatl2_bench.py [--rows 10000000] [--dim 512] [--out profiles/flatl2_bench.json]

One GPU process: run it under a time limit of its own, as above.  At 10M x 512 the shared rows are 20.5 GB, IndexFlatL2's bf16 copy
and half-norms 10.3 GB, the third index's bf16 shadow 10.2 GB.
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
from wise_amd.index.flat_l2 import FlatL2Index  # noqa: E402

NQS = (1, 8, 32, 256)
CROSS = (3, 4, 8, 12, 16, 32)


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
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "flatl2_bench.json"))
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
    l2 = FlatL2Index(d).adopt(X, ids)
    ip = FlatIPIndex(d, shadow=False).adopt(X, ids)
    ipb = FlatIPIndex(d, shadow="bf16").adopt(X, ids)
    torch.cuda.synchronize()
    gq = torch.Generator(device="cuda").manual_seed(2)
    rows = torch.randint(0, N, (max(NQS),), generator=gq, device="cuda")
    Q = torch.nn.functional.normalize(X[rows] + 0.05 * torch.nn.functional.normalize(torch.randn(max(NQS), d, generator=gq, device="cuda"), dim=1),
                                      dim=1).contiguous()
    out = {"what": "tools/flatl2_bench.py: IndexFlatL2 and IndexFlatIP(shadow=False) over the same fp32 tensor, alternating call by call in "
                   "one run; seconds are of one call (median, min, max of `calls` timed calls after warm-up)",
           "rows": N, "dim": d, "k": k, "iters": a.iters, "centres": a.centres, "noise": a.noise, "build_seconds": time.time() - t0,
           "device": torch.cuda.get_device_name(0), "batch_min_rows": l2.BATCH_MIN_ROWS, "batch_min_queries": l2.BATCH_MIN_QUERIES,
           "points": {}}

    # on unit rows L2 and the inner product rank the same: the two answers name the same rows (near-ties aside)
    _, Iip = ip.search_device(Q, k)
    _, Il2 = l2.search_device(Q, k)
    out["same_rows_as_inner_product"] = float(((Iip.unsqueeze(2) == Il2.unsqueeze(1)).any(dim=2).float().sum(dim=1) / k).mean())

    for nq in NQS:
        q = Q[:nq].contiguous()
        res = alternate({"IndexFlatL2": lambda: l2.search_device(q, k), "IndexFlatIP": lambda: ip.search_device(q, k)}, a.iters)
        for r in res.values():
            r["queries_per_second"] = nq / r["median"]
        res["ratio_l2_to_ip"] = res["IndexFlatL2"]["median"] / res["IndexFlatIP"]["median"]
        out["points"][f"nq{nq}"] = res
        show(f"search nq={nq}", {n: r for n, r in res.items() if isinstance(r, dict)})

    def exact_l2(q, D, I, ws):
        def run():
            _lib.check(lib.wise_l2_topk_f32(X.data_ptr(), N, d, q.data_ptr(), q.shape[0], k, ids.data_ptr(), 0, D.data_ptr(), I.data_ptr(),
                                            ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "wise_l2_topk_f32")
        return run

    # the exact scans alone, one query a pass and four: the same bytes, N d 4
    for nq in (1, 4):
        q = Q[:nq].contiguous()
        D = torch.empty(nq, k, dtype=torch.float32, device="cuda")
        I = torch.empty(nq, k, dtype=torch.int64, device="cuda")
        ws = torch.empty(lib.wise_l2_topk_workspace_bytes(N, d, nq, k), dtype=torch.uint8, device="cuda")
        wsi = torch.empty(lib.wise_ip_topk_workspace_bytes(N, d, nq, k), dtype=torch.uint8, device="cuda")

        def scan_ip():
            _lib.check(lib.wise_ip_topk_f32(X.data_ptr(), N, d, q.data_ptr(), nq, k, ids.data_ptr(), 0, D.data_ptr(), I.data_ptr(),
                                            wsi.data_ptr(), wsi.numel(), _lib.stream_ptr()), "wise_ip_topk_f32")
        res = alternate({"wise_l2_topk_f32": exact_l2(q, D, I, ws), "wise_ip_topk_f32": scan_ip}, a.iters)
        for r in res.values():
            r["bytes"] = N * d * 4
            r["bytes_per_second"] = N * d * 4 / r["median"]
        res["ratio_l2_to_ip"] = res["wise_l2_topk_f32"]["median"] / res["wise_ip_topk_f32"]["median"]
        out["points"][f"exact_scan_nq{nq}"] = res
        show(f"exact scan nq={nq}", {n: r for n, r in res.items() if isinstance(r, dict)})

    # the batched passes: both over a bf16 copy of the rows on the matrix cores
    q = Q[:256].contiguous()
    l2.BATCH_MIN_QUERIES = 3                       # from here on search_device of IndexFlatL2 IS the batched search
    res = alternate({"wise_l2_topk_batched": lambda: l2.search_device(q, k), "IndexFlatIP_bf16_batched": lambda: ipb.search_device(q, k)}, a.iters)
    res["ratio_l2_to_ip"] = res["wise_l2_topk_batched"]["median"] / res["IndexFlatIP_bf16_batched"]["median"]
    out["points"]["batched_nq256"] = res
    show("batched nq=256", {n: r for n, r in res.items() if isinstance(r, dict)})

    # the crossover: the batched search beside the exact scan's 4-query passes
    wins = {}
    for nq in CROSS:
        q = Q[:nq].contiguous()
        D = torch.empty(nq, k, dtype=torch.float32, device="cuda")
        I = torch.empty(nq, k, dtype=torch.int64, device="cuda")
        ws = torch.empty(lib.wise_l2_topk_workspace_bytes(N, d, nq, k), dtype=torch.uint8, device="cuda")
        res = alternate({"batched": lambda: l2.search_device(q, k), "exact_scan_passes": exact_l2(q, D, I, ws)}, a.iters)
        out["points"][f"small_batch_nq{nq}"] = res
        show(f"nq={nq}", res)
        wins[nq] = res["batched"]["median"] < res["exact_scan_passes"]["median"]
    out["batched_wins_at"] = {str(nq): w for nq, w in wins.items()}
    out["measured_crossover_batch_size"] = next((nq for nq in CROSS if all(wins[m] for m in CROSS if m >= nq)), None)
    out["hbm_bytes"] = {"IndexFlatL2": {"rows_and_ids": l2.hbm_bytes(), "bf16_copy_and_half_norms": 0 if l2._Xb is None else N * (2 * d + 4)},
                        "IndexFlatIP": {"rows_and_ids": N * (4 * d + 8)}}
    out["batched_counters"] = {"answered_from_lists": l2.batched_counts()[0], "handed_to_exact_scan": l2.batched_counts()[1]}
    print(json.dumps({k_: out[k_] for k_ in ("batched_wins_at", "measured_crossover_batch_size", "hbm_bytes", "batched_counters", "same_rows_as_inner_product")}),
          flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

"""IndexSQfp16 beside IndexFlatIP (default shadows) on the same rows, the same box, the same run: bytes held,
queries/s at nq = 1 and nq = 256, the exact scan's bytes/s against N d 2, the batched search's counters and recall@10 against the
fp32 answer.

One seeded clustered set is generated on the device chunk by chunk (tools/ivfsqfp16_bench.py's recipe); IndexFlatIP takes the fp32
rows, IndexSQfp16 encodes the same chunks (the fp32 form of ITS index never exists in HBM).  Timing: every shape of both indexes is
warmed up first (IndexFlatIP builds its shadows then); then the two indexes ALTERNATE call by call — round r times one call of
each, HIP events around the single call — for --iters rounds (at least 10), so that clock and thermal drift fall on both alike; a
point reports the median with the smallest and the largest call (the spread).  The exact scan is also timed alone (nq = 1 through
wise_ipsq16_topk whatever the routing) and its bytes/s = N d 2 / median reported, and at nq = 3, 8 and 32 the batched search is
timed beside the exact scan's 4-query passes: where the two cross is what the batch-size floor of the routing follows
(FlatSQfp16IPIndex.BATCH_MIN_QUERIES).  There is no pass mark: the expectation (README) is derived — a batched pass reads the bytes
the bf16 shadow pass reads, a single query about twice the int8 shadow's.

    timeout 1100 python tools/sqfp16_bench.py [--rows 10000000] [--dim 512] [--out profiles/sqfp16_bench.json]

One GPU process: run it under a time limit of its own, as above.  At 10M x 512 IndexFlatIP holds 20.5 GB of rows and builds 5.2 GB
(int8) and 10.2 GB (bf16) of shadows; IndexSQfp16 holds 10.2 GB.
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
from wise_amd.index.flat_sq import FlatSQfp16IPIndex  # noqa: E402

NQS = (1, 256)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--centres", type=int, default=4096)
    ap.add_argument("--noise", type=float, default=0.35)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "sqfp16_bench.json"))
    a = ap.parse_args()
    if a.iters < 10:
        ap.error("--iters must be at least 10")
    N, d, k = a.rows, a.dim, a.k
    lib = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(1)
    centres = torch.nn.functional.normalize(torch.randn(a.centres, d, generator=g, device="cuda"), dim=1)
    flat = FlatIPIndex(d)                      # default shadows: int8 for single queries, bf16 for the batched passes
    sq16 = FlatSQfp16IPIndex(d)
    flat.reserve(N)
    sq16.reserve(N)
    t0 = time.time()
    step = 1 << 19
    for s in range(0, N, step):
        n = min(step, N - s)
        x = chunk(centres, a.noise, n, g)
        ids = torch.arange(s, s + n, device="cuda", dtype=torch.int64)
        flat.add_with_ids(x, ids)
        sq16.add_with_ids(x, ids)
    torch.cuda.synchronize()
    gq = torch.Generator(device="cuda").manual_seed(2)
    rows = torch.randint(0, N, (max(NQS),), generator=gq, device="cuda")
    Q = torch.nn.functional.normalize(flat._X[rows] + 0.05 * torch.nn.functional.normalize(torch.randn(max(NQS), d, generator=gq, device="cuda"), dim=1),
                                      dim=1).contiguous()
    out = {"what": "tools/sqfp16_bench.py: IndexSQfp16 and IndexFlatIP (default shadows) alternating call by call in one run; seconds are "
                   "of one search_device call (median, min, max of `calls` timed calls after warm-up)",
           "rows": N, "dim": d, "k": k, "iters": a.iters, "centres": a.centres, "noise": a.noise, "build_seconds": time.time() - t0,
           "device": torch.cuda.get_device_name(0), "batch_min_rows": sq16.BATCH_MIN_ROWS, "points": {}}

    # recall@k of IndexSQfp16 against the fp32 answer (the fp32 scan itself: shadows off for this call), and the counters
    exact = FlatIPIndex(d, shadow=False).adopt(flat._X, flat._ids)
    _, If = exact.search_device(Q, k)
    _, I16 = sq16.search_device(Q, k)
    same = (If.unsqueeze(2) == I16.unsqueeze(1)).any(dim=2).float().sum(dim=1) / k
    out["recall_at_k_vs_fp32"] = float(same.mean())
    del exact

    for nq in NQS:
        q = Q[:nq].contiguous()
        res = alternate({"IndexSQfp16": lambda: sq16.search_device(q, k), "IndexFlatIP": lambda: flat.search_device(q, k)}, a.iters)
        for name, r in res.items():
            r["queries_per_second"] = nq / r["median"]
        out["points"][f"nq{nq}"] = res
        print(f"nq={nq}: " + ", ".join(f"{n} {r['median'] * 1e3:.3f} ms [{r['min'] * 1e3:.3f}, {r['max'] * 1e3:.3f}] = {r['queries_per_second']:.0f} q/s"
                                       for n, r in res.items()), flush=True)

    # the exact scan alone, one query a pass and four: bytes/s against N d 2
    for nq in (1, 4):
        q = Q[:nq].contiguous()
        D = torch.empty(nq, k, dtype=torch.float32, device="cuda")
        I = torch.empty(nq, k, dtype=torch.int64, device="cuda")
        ws = torch.empty(lib.wise_ipsqfp16_topk_workspace_bytes(N, d, nq, k), dtype=torch.uint8, device="cuda")

        def scan():
            _lib.check(lib.wise_ipsq16_topk(sq16._H.data_ptr(), N, d, q.data_ptr(), nq, k, sq16._ids.data_ptr(), 0, D.data_ptr(), I.data_ptr(),
                                            ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "wise_ipsq16_topk")
        r = alternate({"scan": scan}, a.iters)["scan"]
        r["bytes"] = N * d * 2
        r["bytes_per_second"] = N * d * 2 / r["median"]
        out["points"][f"exact_scan_nq{nq}"] = r
        print(f"exact scan nq={nq}: {r['median'] * 1e3:.3f} ms [{r['min'] * 1e3:.3f}, {r['max'] * 1e3:.3f}] = {r['bytes_per_second'] / 1e12:.2f} TB/s of N d 2", flush=True)

    # small batches: the batched search (what search_device routes nq >= 3 to at this size) beside the exact scan's 4-query passes
    for nq in (3, 8, 32):
        q = Q[:nq].contiguous()
        D = torch.empty(nq, k, dtype=torch.float32, device="cuda")
        I = torch.empty(nq, k, dtype=torch.int64, device="cuda")
        ws = torch.empty(lib.wise_ipsqfp16_topk_workspace_bytes(N, d, nq, k), dtype=torch.uint8, device="cuda")

        def passes():
            _lib.check(lib.wise_ipsq16_topk(sq16._H.data_ptr(), N, d, q.data_ptr(), nq, k, sq16._ids.data_ptr(), 0, D.data_ptr(), I.data_ptr(),
                                            ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "wise_ipsq16_topk")
        sq16.BATCH_MIN_QUERIES = 3                 # this point times the batched search itself, whatever the class would route
        res = alternate({"batched": lambda: sq16.search_device(q, k), "exact_scan_passes": passes}, a.iters)
        out["points"][f"small_batch_nq{nq}"] = res
        print(f"nq={nq}: " + ", ".join(f"{n} {r['median'] * 1e3:.3f} ms [{r['min'] * 1e3:.3f}, {r['max'] * 1e3:.3f}]" for n, r in res.items()), flush=True)

    out["hbm_bytes"] = {"IndexSQfp16": sq16.hbm_bytes(),
                        "IndexFlatIP": {"rows_and_ids": N * (4 * d + 8), "int8_shadow": 0 if flat._Xq is None else N * (d + 4),
                                        "bf16_shadow": 0 if flat._Xb is None else N * d * 2}}
    fb = out["hbm_bytes"]["IndexFlatIP"]
    out["hbm_ratio"] = sq16.hbm_bytes() / (fb["rows_and_ids"] + fb["int8_shadow"] + fb["bf16_shadow"])
    out["batched_counters"] = {"answered_from_lists": sq16.batched_counts()[0], "handed_to_exact_scan": sq16.batched_counts()[1]}
    out["flat_shadow_counters"] = {"answered_from_shadow": flat.shadow_counts()[0], "handed_to_fp32_scan": flat.shadow_counts()[1]}
    print(json.dumps({k_: out[k_] for k_ in ("hbm_bytes", "hbm_ratio", "batched_counters", "flat_shadow_counters", "recall_at_k_vs_fp32")}), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

"""search_grouped beside the same index's exact top-k scan, the same box, the same run (README.md): IndexSQ8bit and
IndexFlatIP(shadow=False) at nq = 1 and 4, k = 10, over groups that are contiguous runs of rows (mean length --run, a flat index
holding a video's frames in store order) and over the same keys permuted over the rows.

One seeded clustered set is generated on the device chunk by chunk (tools/sq8_bench.py's recipe).  IndexFlatIP adopts the fp32
tensor; IndexSQ8bit trains its ranges over every row and encodes on the GPU.  Timing: every callable is warmed up first; then the
callables of a point ALTERNATE call by call — HIP events around the single call — for --iters rounds (at least 10), so that clock
and thermal drift fall on all alike; a point reports the median with the smallest and the largest call (the spread), and the ratio
of each grouped search to the exact scan of the same point.  The three stages of a grouped search are also timed one by one (the
score pass, wise_group_best, wise_group_topk), so that a ratio far from the derived one names its stage.

Derived: a grouped search reads the exact scan's bytes plus about 12 N + 8 G bytes a query (+2 % of IndexSQ8bit's N d at d = 512).
There is no pass mark.

    timeout 900 python tools/group_bench.py [--rows 10000000] [--dim 512] [--out profiles/group_bench.json]

One GPU process: run it under a time limit of its own, as above.  At 10M x 512 the fp32 rows are 20.5 GB and the codes 5.1 GB.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from wise_amd import _lib  # noqa: E402
from wise_amd.index.flat_ip import FlatIPIndex  # noqa: E402
from wise_amd.index.flat_sq import FlatSQ8IPIndex  # noqa: E402
from wise_amd.index.group_search import workspace_regions  # noqa: E402

NQS = (1, 4)


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
    print(f"{tag}: " + ", ".join(f"{n} {r['median'] * 1e3:.3f} ms [{r['min'] * 1e3:.3f}, {r['max'] * 1e3:.3f}]" for n, r in res.items()
                                 if isinstance(r, dict) and "median" in r), flush=True)


def stage_calls(lib, ix, q, k):
    """the three stages of search_grouped_device on the index's present tables, as three callables over one workspace"""
    t, N, d, nq, st = ix._group_tables(), ix.ntotal, ix.d, q.shape[0], _lib.stream_ptr()
    G = int(t["keys"].numel())
    ws = torch.empty(lib.wise_group_workspace_bytes(N, G, nq, k), dtype=torch.uint8, device="cuda")
    best_at, part_at = workspace_regions(nq, N, G)
    D = torch.empty(nq, k, dtype=torch.float32, device="cuda")
    I = torch.empty(nq, k, dtype=torch.int64, device="cuda")
    Gk = torch.empty(nq, k, dtype=torch.int64, device="cuda")
    fn = getattr(lib, ix._GROUP_SCORES)

    def scores():
        operands = ix._group_operands(lib, q)
        _lib.check(fn(_lib.ptr(ix._store.rows), N, d, *(o.data_ptr() for o in operands), nq, 0, ws.data_ptr(), st), ix._GROUP_SCORES)

    def best():
        _lib.check(lib.wise_group_best(ws.data_ptr(), N, nq, t["off"].data_ptr(), t["rows"].data_ptr(), G, ws.data_ptr() + best_at, st),
                   "wise_group_best")

    def topk():
        _lib.check(lib.wise_group_topk(ws.data_ptr() + best_at, G, nq, k, t["gid"].data_ptr(), N, t["keys"].data_ptr(), _lib.ptr(ix._store.ids),
                                       ix._store.id_base, 0, D.data_ptr(), I.data_ptr(), Gk.data_ptr(), ws.data_ptr() + part_at,
                                       ws.numel() - part_at, st), "wise_group_topk")
    return {"stage1_scores": scores, "stage2_group_best": best, "stage3_group_topk": topk}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--run", type=int, default=200, help="mean rows of a group")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--centres", type=int, default=4096)
    ap.add_argument("--noise", type=float, default=0.35)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "group_bench.json"))
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
    flat = FlatIPIndex(d, shadow=False).adopt(X, ids)
    sq8 = FlatSQ8IPIndex(d)
    sq8.train(X)
    sq8.reserve(N)
    for s in range(0, N, step):
        sq8.add_with_ids(X[s:s + step], ids[s:s + step])
    torch.cuda.synchronize()
    gq = torch.Generator(device="cuda").manual_seed(2)
    rows = torch.randint(0, N, (max(NQS),), generator=gq, device="cuda")
    Q = torch.nn.functional.normalize(X[rows] + 0.05 * torch.nn.functional.normalize(torch.randn(max(NQS), d, generator=gq, device="cuda"), dim=1),
                                      dim=1).contiguous()
    # groups: runs of uneven length, mean --run (cut points drawn without replacement), and the same keys permuted over the rows
    rng = np.random.default_rng(3)
    G = max(1, N // a.run)
    cuts = np.sort(rng.choice(np.arange(1, N), size=G - 1, replace=False)) if G > 1 else np.empty(0, dtype=np.int64)
    runs = np.searchsorted(cuts, np.arange(N), side="right").astype(np.int64)
    layouts = {"contiguous": runs, "permuted": rng.permutation(runs)}
    host_ids = np.arange(N, dtype=np.int64)
    out = {"what": "tools/group_bench.py: search_grouped and the same index's exact top-k scan alternating call by call in one run; seconds "
                   "are of one call (median, min, max of `calls` timed calls after warm-up); ratio = grouped median / exact median",
           "rows": N, "dim": d, "k": k, "groups": G, "mean_run": a.run, "iters": a.iters, "centres": a.centres, "noise": a.noise,
           "build_seconds": time.time() - t0, "device": torch.cuda.get_device_name(0),
           "derived_extra_bytes_per_query": 12 * N + 8 * G, "points": {}}
    for name, ix in (("IndexSQ8bit", sq8), ("IndexFlatIP_shadow_off", flat)):
        scan_bytes = N * d * (1 if ix is sq8 else 4)
        for layout, gid in layouts.items():
            t1 = time.time()
            ix.set_groups(host_ids, gid)
            set_groups_seconds = time.time() - t1
            for nq in NQS:
                q = Q[:nq].contiguous()
                res = alternate({"grouped": lambda: ix.search_grouped_device(q, k), "exact": lambda: ix.search_device(q, k)}, a.iters)
                res["ratio"] = res["grouped"]["median"] / res["exact"]["median"]
                res["derived_ratio"] = 1.0 + (12 * N + 8 * G) / scan_bytes
                res["stages"] = alternate(stage_calls(lib, ix, q, k), a.iters)
                res["set_groups_seconds"] = set_groups_seconds
                out["points"][f"{name}_{layout}_nq{nq}"] = res
                show(f"{name} {layout} nq={nq} ratio {res['ratio']:.3f} (derived {res['derived_ratio']:.3f})", res)
                show("   stages", res["stages"])
        ix.clear_groups()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

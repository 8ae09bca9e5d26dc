""""Search inside these videos": resolving a GROUP selector on the device beside the route that existed before it — the media ids
expanded into vector ids on the host and resolved as an IDSelectorBatch — the same box, the same run (README.md).

One IndexSQ8bit over --rows x --dim seeded clustered rows (tools/sq8_bench.py's recipe, encoded chunk by chunk: 5.1 GB of codes at
10M x 512, no fp32 copy is kept), --rows / --run groups that are contiguous runs of uneven length (a video's frames in store order),
and per selectivity (1 %, 10 %, 50 % of the groups) a fresh draw of keys.  Timed, each from HOST keys, a new selector object per
call (every REST request carries a new filter, so nothing is cached), wall clock around the call and a device synchronize:
  (a) groups  IDSelectorGroups(keys).resolve(index): the keys sorted on the host, copied, wise_sel_bitmap_groups (two launches)
  (b) batch   the parent route: the keys expanded to vector ids through a host copy of the group tables (group_off / group_rows: one
              concatenation of ranges, no search), then IDSelectorBatch(ids).resolve(index) — the copy of 8 bytes per selected vector,
              torch.sort on the device and one binary search per row; `expand` is the host part alone
  (c) search  the filtered top-k search that follows, on the bitmap of (a) and on the bitmap of (b): the same search (the two bitmaps
              are asserted equal, and so are the answers)
(a) and (b) ALTERNATE call by call for --iters rounds (at least 10) after a warm-up; a point reports the median with the smallest and
the largest call.  Derived, not measured: (a) moves 4 N + N / 8 bytes of HBM whatever the selectivity; (b) moves 8 bytes per selected
vector over PCIe.  There is no pass mark.

    timeout 900 python tools/sel_tree_bench.py [--rows 10000000] [--dim 512] [--out profiles/sel_tree_bench.json]

One GPU process: run it under a time limit of its own, as above.
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
from wise_amd.index.flat_sq import FlatSQ8IPIndex  # noqa: E402
from wise_amd.index.selector import IDSelectorBatch, IDSelectorGroups  # noqa: E402

SHARES = (0.01, 0.10, 0.50)


def chunk(centres, noise, n, g):
    d = centres.shape[1]
    pick = torch.randint(0, centres.shape[0], (n,), generator=g, device="cuda")
    z = torch.nn.functional.normalize(torch.randn(n, d, generator=g, device="cuda"), dim=1)
    return torch.nn.functional.normalize(centres[pick] + noise * z, dim=1).contiguous()


def wall_seconds(fn):
    """one call from the host's point of view: everything it enqueued has finished"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def alternate(fns: dict, iters: int, warmup: int = 2) -> dict:
    """name -> {median, min, max} seconds of one call, the callables taking turns round by round"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    times = {name: [] for name in fns}
    for _ in range(iters):
        for name, fn in fns.items():
            times[name].append(wall_seconds(fn)[0])
    return {name: {"median": statistics.median(t), "min": min(t), "max": max(t), "calls": len(t)} for name, t in times.items()}


def show(tag, res):
    print(f"{tag}: " + ", ".join(f"{n} {r['median'] * 1e3:.3f} ms [{r['min'] * 1e3:.3f}, {r['max'] * 1e3:.3f}]" for n, r in res.items()
                                 if isinstance(r, dict) and "median" in r), flush=True)


def expand(keys, group_keys, group_off, group_rows, row_ids):
    """the vector ids of the groups `keys` from host tables: the ranges group_rows[off[g] : off[g + 1]] laid end to end"""
    g = np.searchsorted(group_keys, keys)
    g = g[(g < group_keys.size) & (group_keys[np.minimum(g, group_keys.size - 1)] == keys)]
    lo, n = group_off[g], group_off[g + 1] - group_off[g]
    start = np.repeat(lo - np.concatenate([[0], np.cumsum(n)[:-1]]), n)
    return row_ids[group_rows[start + np.arange(int(n.sum()), dtype=np.int64)]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--run", type=int, default=200, help="mean rows of a group")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--centres", type=int, default=4096)
    ap.add_argument("--noise", type=float, default=0.35)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "sel_tree_bench.json"))
    a = ap.parse_args()
    if a.iters < 10:
        ap.error("--iters must be at least 10")
    N, d, k = a.rows, a.dim, a.k
    g = torch.Generator(device="cuda").manual_seed(1)
    centres = torch.nn.functional.normalize(torch.randn(a.centres, d, generator=g, device="cuda"), dim=1)
    t0 = time.time()
    step = 1 << 19
    ix = FlatSQ8IPIndex(d)
    ix.reserve(N)
    q = None
    for s in range(0, N, step):
        n = min(step, N - s)
        x = chunk(centres, a.noise, n, g)
        if s == 0:                                        # unit rows: the ranges of the first chunk serve every chunk (values outside clamp)
            ix.train(x)
            q = x[:1].clone()
        ix.add_with_ids(x, torch.arange(s, s + n, device="cuda", dtype=torch.int64))
    torch.cuda.synchronize()
    # groups: runs of uneven length, mean --run (cut points drawn without replacement); keys with gaps
    rng = np.random.default_rng(3)
    G = max(1, N // a.run)
    cuts = np.sort(rng.choice(np.arange(1, N), size=G - 1, replace=False)) if G > 1 else np.empty(0, dtype=np.int64)
    key_of_row = np.searchsorted(cuts, np.arange(N), side="right").astype(np.int64) * 3 + 5
    row_ids = np.arange(N, dtype=np.int64)
    ix.set_groups(row_ids, key_of_row)
    t = ix._group_tables()                                # a host copy of the tables: what the caller of route (b) expands with
    group_keys, group_off = t["keys"].cpu().numpy(), t["off"].cpu().numpy()
    group_rows = t["rows"].cpu().numpy().view(np.uint32).astype(np.int64)
    out = {"what": "tools/sel_tree_bench.py: from host keys to a bitmap over the rows — (a) `groups`, IDSelectorGroups(keys).resolve(index), "
                   "and (b) `batch`, the keys expanded to vector ids on the host (`expand` is that part alone) and IDSelectorBatch(ids)"
                   ".resolve(index), copy included — alternating call by call in one run, a new selector per call; and (c) the filtered "
                   "top-k search on either bitmap; wall-clock seconds of one call with a device synchronize (median, min, max of `calls` "
                   "calls after warm-up); ratio = batch median / groups median",
           "index": "IndexSQ8bit", "rows": N, "dim": d, "k": k, "groups": G, "mean_run": a.run, "iters": a.iters, "centres": a.centres,
           "noise": a.noise, "build_seconds": time.time() - t0, "device": torch.cuda.get_device_name(0),
           "derived_groups_hbm_bytes": 4 * N + N // 8, "points": {}}
    for share in SHARES:
        keys = rng.permutation(group_keys)[:max(1, int(round(share * G)))].copy()
        ids = expand(keys, group_keys, group_off, group_rows, row_ids)
        by_groups = IDSelectorGroups(keys).resolve(ix)
        by_batch = IDSelectorBatch(ids).resolve(ix)
        assert torch.equal(by_groups.bitmap, by_batch.bitmap), share
        res = alternate({"groups": lambda: IDSelectorGroups(keys).resolve(ix),
                         "batch": lambda: IDSelectorBatch(expand(keys, group_keys, group_off, group_rows, row_ids)).resolve(ix),
                         "expand": lambda: expand(keys, group_keys, group_off, group_rows, row_ids)}, a.iters)
        res["ratio"] = res["batch"]["median"] / res["groups"]["median"]
        res["selected_groups"], res["selected_rows"] = int(keys.size), int(ids.size)
        res["derived_batch_pcie_bytes"] = 8 * int(ids.size)
        Da, Ia = ix.search_device(q, k, sel=by_groups)
        Db, Ib = ix.search_device(q, k, sel=by_batch)
        assert torch.equal(Da, Db) and torch.equal(Ia, Ib), share
        res["search"] = alternate({"after_groups": lambda: ix.search_device(q, k, sel=by_groups),
                                   "after_batch": lambda: ix.search_device(q, k, sel=by_batch)}, a.iters)
        out["points"][f"share_{share:g}"] = res
        show(f"{share:.0%} of the groups ({ids.size} rows) batch / groups {res['ratio']:.2f}", res)
        show("   search", res["search"])
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

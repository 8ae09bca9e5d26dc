"""IndexIVFFlatL2 beside IndexIVFFlat and IndexFlatL2 on the same rows, the same box, the same run: queries/s, the
second stage alone, and recall@10 against IndexFlatL2's exact answer.

One seeded clustered set is generated on the device (tools/ivfsq_bench.py's recipe) and every row is given a length log-uniform over
[1, --spread]: the rows are not normalised.  IndexIVFFlatL2 trains its plain k-means and IndexIVFFlat its spherical one on the same
sample; IndexFlatL2 holds the same rows and gives the exact answer.  Per nprobe in {32, 1024} and nq in {1, 256}: the time of whole
`search_device` calls of all three, and of the second stage alone of the two inverted-file types (the probes computed once and
handed back to the index, so what is timed is everything after the coarse stage).  Timing: every shape of every index is warmed up
first; then the indexes ALTERNATE — round r times one call of each, HIP events around the single call — for --iters rounds (at
least 10), so that clock and thermal drift fall on all alike; a point reports the median with the smallest and the largest call.
What to expect is derived, not measured: wise_ivfl2_scan reads the bytes wise_ivf_scan_f32 reads, N_probed d 4, so the second stage
at nq = 256, nprobe 1024 should sit near IndexIVFFlat's of this run (the lists differ: two k-means over rows that are not
normalised fill their cells differently, so N_probed is reported for both).  No ratio is fixed in advance.

    timeout 1100 python tools/ivfl2_bench.py [--rows 10000000] [--dim 512] [--out profiles/ivfl2_bench.json]

One GPU process: run it under a time limit of its own, as above.  At 10M x 512 the three indexes take about 62 GB of HBM, and merging
an inverted-file index's lists needs about 40 GB more for a moment.
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
from wise_amd.index.flat_l2 import FlatL2Index  # noqa: E402
from wise_amd.index.ivf_flat import IVFFlatIPIndex, IVFFlatL2Index, reference_nlist  # noqa: E402

NPROBES = (32, 1024)
NQS = (1, 256)


def chunk(centres, noise, spread, n, g):
    d = centres.shape[1]
    pick = torch.randint(0, centres.shape[0], (n,), generator=g, device="cuda")
    z = torch.nn.functional.normalize(torch.randn(n, d, generator=g, device="cuda"), dim=1)
    u = torch.nn.functional.normalize(centres[pick] + noise * z, dim=1)
    length = torch.exp(torch.rand(n, 1, generator=g, device="cuda") * float(np.log(spread)))
    return (u * length).contiguous()


def one_call_seconds(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def alternate(fns: dict, iters: int, warmup: int = 2) -> dict:
    """name -> {median, min, max} seconds of one call, the callables taking turns round by round"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(iters):
        for name, fn in fns.items():
            times[name].append(one_call_seconds(fn))
    return {name: {"median": statistics.median(t), "min": min(t), "max": max(t)} for name, t in times.items()}


def recall(I, If):
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / len(b) for a, b in zip(I, If)]))


def clock():
    torch.cuda.synchronize()
    return time.time()


class FixedProbes:
    """search_device with the coarse stage's answer computed once and handed back: the time of everything after it"""

    def __init__(self, index, q, k):
        self.index, self.q, self.k = index, q, k
        self.probes = index.probes_device(q, index._clamped_nprobe()).contiguous()

    def probed_rows(self):
        """mean rows of the probed lists per query: N_probed"""
        off = self.index._lists.list_off
        p = self.probes.clamp(min=0)
        return float(((off[p + 1] - off[p]) * (self.probes >= 0)).sum(dim=1).double().mean().item())

    def __call__(self):
        coarse = self.index._coarse
        real = coarse.probes_device
        coarse.probes_device = lambda qs, nprobe: self.probes
        try:
            return self.index.search_device(self.q, self.k)
        finally:
            coarse.probes_device = real


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--noise", type=float, default=0.35)
    ap.add_argument("--spread", type=float, default=4.0)
    ap.add_argument("--out", default="profiles/ivfl2_bench.json")
    args = ap.parse_args()
    if args.iters < 10:
        ap.error("--iters: at least 10 timed calls per point")
    N, d, k = args.rows, args.dim, 10
    nlist = reference_nlist(N)
    g = torch.Generator(device="cuda").manual_seed(0)
    centres = torch.nn.functional.normalize(torch.randn(max(nlist // 2, 16), d, generator=g, device="cuda"), dim=1)
    g = torch.Generator(device="cuda").manual_seed(1)
    train = chunk(centres, args.noise, args.spread, min(N, 100 * nlist), g)
    ivf_names = ["IndexIVFFlatL2", "IndexIVFFlat"]
    idx = dict(zip(ivf_names, (IVFFlatL2Index(d, nlist), IVFFlatIPIndex(d, nlist))))
    train_s = {}
    for name, i in idx.items():
        t0 = clock()
        i.train(train)
        train_s[name] = clock() - t0
    del train
    print(f"{N} x {d}, nlist {nlist}: train {json.dumps(train_s)}", flush=True)
    exact, add_s, Q = FlatL2Index(d), dict.fromkeys(ivf_names, 0.0), None
    exact.reserve(N)
    g = torch.Generator(device="cuda").manual_seed(2)
    for s in range(0, N, 1 << 20):
        x = chunk(centres, args.noise, args.spread, min(1 << 20, N - s), g)
        ids = torch.arange(s, s + x.shape[0], dtype=torch.int64, device="cuda")
        exact.add_with_ids(x, ids)
        for name, i in idx.items():
            t0 = clock()
            i.add_with_ids(x, ids)
            add_s[name] += clock() - t0
        if Q is None:      # queries: perturbed rows of the set
            e = torch.nn.functional.normalize(torch.randn(256, d, generator=g, device="cuda"), dim=1)
            Q = (x[:256] + 0.05 * x[:256].norm(dim=1, keepdim=True) * e).contiguous()
    for name, i in idx.items():
        t0 = clock()
        i._finalize()
        add_s[name] += clock() - t0
        torch.cuda.empty_cache()
    sizes = {name: (i._lists.list_off[1:] - i._lists.list_off[:-1]).double() for name, i in idx.items()}
    out = {"device": torch.cuda.get_device_name(0), "rows": N, "dim": d, "nlist": nlist, "k": k, "iters": args.iters, "noise": args.noise,
           "spread": args.spread,
           "timing": "the indexes alternate call by call; seconds of one call: median, min, max over iters calls",
           "train_seconds": train_s, "add_seconds": add_s,
           "list_sizes": {name: {"empty": int((s == 0).sum().item()), "max": int(s.max().item()), "mean": float(s.mean().item()),
                                 "std": float(s.std().item())} for name, s in sizes.items()},
           "points": []}
    _, If = exact.search_device(Q, k)
    If = If.cpu().numpy()
    all_names = ivf_names + ["IndexFlatL2"]
    for nprobe in NPROBES:
        for i in idx.values():
            i.nprobe = nprobe
        rec = {"IndexIVFFlatL2": recall(idx["IndexIVFFlatL2"].search_device(Q, k)[1].cpu().numpy(), If)}
        for nq in NQS:
            q = Q[:nq].contiguous()
            fns = {name: (lambda i=i: i.search_device(q, k)) for name, i in idx.items()}
            fns["IndexFlatL2"] = lambda: exact.search_device(q, k)
            whole = alternate(fns, args.iters)
            fixed = {name: FixedProbes(i, q, k) for name, i in idx.items()}
            stage2 = alternate(fixed, args.iters)
            for name in all_names:
                point = {"index": name, "nprobe": nprobe if name in idx else None, "nq": nq, "search_seconds": whole[name],
                         "queries_per_s": nq / whole[name]["median"]}
                if name in idx:
                    point["second_stage_seconds"] = stage2[name]
                    point["probed_rows_per_query"] = fixed[name].probed_rows()
                    point["second_stage_bytes_per_s"] = point["probed_rows_per_query"] * nq * d * 4 / stage2[name]["median"]
                if name in rec:
                    point["recall_at_10_vs_flat_l2"] = rec[name]
                print(json.dumps(point), flush=True)
                out["points"].append(point)
            a, b = (stage2[n]["median"] for n in ivf_names)
            pa, pb = (fixed[n].probed_rows() for n in ivf_names)
            out[f"second_stage_time_ratio_ivfflatl2_over_ivfflat_nprobe{nprobe}_nq{nq}"] = a / b
            out[f"probed_rows_ratio_ivfflatl2_over_ivfflat_nprobe{nprobe}_nq{nq}"] = pa / pb
            out[f"whole_search_time_ratio_ivfflatl2_over_ivfflat_nprobe{nprobe}_nq{nq}"] = whole[ivf_names[0]]["median"] / whole[ivf_names[1]]["median"]
            out[f"whole_search_time_ratio_flatl2_over_ivfflatl2_nprobe{nprobe}_nq{nq}"] = whole["IndexFlatL2"]["median"] / whole[ivf_names[0]]["median"]
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({k_: v for k_, v in out.items() if "ratio" in k_}))
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()

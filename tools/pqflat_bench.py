"""IndexPQ<m> and IndexPQ<m>R8 beside IndexSQ8bit, IndexFlatIP (default shadows) and IndexIVFPQ<m>R8 (nprobe 1024) on the same rows, the
same box, the same run (README.md): bytes held, the time of one search call at nq = 1, 4, 32 and 256, the stages of
the R form on their own (tables, scan, re-ranking), the time of a scan pass carrying 1, 2 and 4 queries, and recall@10 against the
fp32 answer.

One seeded clustered set is generated on the device chunk by chunk (tools/sq8_bench.py's recipe).  IndexFlatIP adopts the fp32
tensor; the other types encode it on the GPU (IndexSQ8bit trains its ranges over every row, the PQ types their codebooks on the seeded
sample their classes draw, IndexIVFPQ<m>R8 its coarse quantizer on min(N, 100 nlist) rows).  Timing: every shape is warmed up first;
then the callables of a point ALTERNATE call by call — HIP events around the single call — for --iters rounds (at least 10), so that
clock and thermal drift fall on all alike; a point reports the median with the smallest and the largest call (the spread).

The single-query scan is set beside two DERIVED floors: the code bytes at the HBM rate IndexSQ8bit's scan reaches in the same run, and
N m table lookups at 32 conflict-free ds_read_b32 per clock per CU.  There is no pass mark.

    timeout 1100 python tools/pqflat_bench.py [--rows 10000000] [--dim 512] [--m 64] [--out profiles/pqflat_bench.json]

One GPU process: run it under a time limit of its own, as above.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sq8_bench import alternate, chunk, show  # noqa: E402
from wise_amd import _lib  # noqa: E402
from wise_amd.index.flat_ip import FlatIPIndex  # noqa: E402
from wise_amd.index.flat_pq import FlatPQIPIndex, FlatPQRefineIPIndex  # noqa: E402
from wise_amd.index.flat_sq import FlatSQ8IPIndex  # noqa: E402
from wise_amd.index.ivf_flat import reference_nlist  # noqa: E402
from wise_amd.index.ivf_pq import IVFPQRefineIPIndex  # noqa: E402

NQS = (1, 4, 32, 256)
CUS, LOOKUPS_PER_CLOCK_PER_CU = 256, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--centres", type=int, default=4096)
    ap.add_argument("--noise", type=float, default=0.35)
    ap.add_argument("--nprobe", type=int, default=1024)
    ap.add_argument("--clock-ghz", type=float, default=2.4, help="shader clock the derived lookup floor assumes")
    ap.add_argument("--no-ivf", action="store_true", help="leave IndexIVFPQ<m>R8 out")
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "pqflat_bench.json"))
    a = ap.parse_args()
    if a.iters < 10:
        ap.error("--iters must be at least 10")
    N, d, m, k = a.rows, a.dim, a.m, a.k
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
    sq8 = FlatSQ8IPIndex(d)
    sq8.train(X)
    sq8.reserve(N)
    pq = FlatPQIPIndex(d, m)
    t1 = time.time()
    pq.train(X)                                # rows perm[:65536] of the seeded permutation
    torch.cuda.synchronize()
    train_seconds = time.time() - t1
    pq.reserve(N)
    r8 = FlatPQRefineIPIndex(d, m, 8)
    r8.set_codebooks(pq.codebooks)
    r8.reserve(N)
    ivf = None
    if not a.no_ivf:
        nlist = reference_nlist(N)
        ivf = IVFPQRefineIPIndex(d, nlist, m, 8)
        t1 = time.time()
        ivf.train(X[torch.randperm(N, generator=g, device="cuda")[:min(N, 100 * nlist)]])
        torch.cuda.synchronize()
        ivf_train_seconds = time.time() - t1
        ivf.nprobe = a.nprobe
    for s in range(0, N, step):
        xs, is_ = X[s:s + step], ids[s:s + step]
        sq8.add_with_ids(xs, is_)
        pq.add_with_ids(xs, is_)
        r8.add_with_ids(xs, is_)
        if ivf is not None:
            ivf.add_with_ids(xs, is_)
    torch.cuda.synchronize()
    gq = torch.Generator(device="cuda").manual_seed(2)
    rows = torch.randint(0, N, (max(NQS),), generator=gq, device="cuda")
    Q = torch.nn.functional.normalize(X[rows] + 0.05 * torch.nn.functional.normalize(torch.randn(max(NQS), d, generator=gq, device="cuda"), dim=1),
                                      dim=1).contiguous()
    types = {f"IndexPQ{m}": pq, f"IndexPQ{m}R8": r8, "IndexSQ8bit": sq8, "IndexFlatIP": flat}
    if ivf is not None:
        types[f"IndexIVFPQ{m}R8"] = ivf
    out = {"what": "tools/pqflat_bench.py: " + ", ".join(types) + " alternating call by call in one run; seconds are of one call (median, "
                   "min, max of `calls` timed calls after warm-up)",
           "rows": N, "dim": d, "m": m, "k": k, "iters": a.iters, "centres": a.centres, "noise": a.noise, "build_seconds": time.time() - t0,
           "codebook_train_seconds": train_seconds, "device": torch.cuda.get_device_name(0), "k_factor": r8.k_factor, "points": {}}
    if ivf is not None:
        out.update(nlist=ivf.nlist, nprobe=a.nprobe, ivf_train_seconds=ivf_train_seconds)

    # recall@k against the fp32 answer (the fp32 scan itself: shadows off for this call)
    exact = FlatIPIndex(d, shadow=False).adopt(flat._X, flat._ids)
    _, If = exact.search_device(Q, k)
    recall = {}
    for name, idx in types.items():
        _, I = idx.search_device(Q, k)
        recall[name] = float(((I.unsqueeze(2) == If.unsqueeze(1)).any(dim=2).float().sum(dim=1) / k).mean())
    out["recall_at_k_vs_fp32"] = recall
    del exact

    for nq in NQS:
        q = Q[:nq].contiguous()
        res = alternate({name: (lambda idx=idx: idx.search_device(q, k)) for name, idx in types.items()}, a.iters)
        for r in res.values():
            r["queries_per_second"] = nq / r["median"]
        out["points"][f"nq{nq}"] = res
        show(f"search nq={nq}", res)

    # the stages of the R form on their own, and a scan pass carrying 1, 2 and 4 queries
    C, rows8, scales8 = r8._codes_t, r8._xrows, r8._xscales
    for nq in (1, 2, 4, 32):
        q = Q[:nq].contiguous()
        kc = r8.candidates(k)
        lut = torch.empty(nq, m, 256, dtype=torch.float32, device="cuda")
        cD = torch.empty(nq, kc, dtype=torch.float32, device="cuda")
        cand = torch.empty(nq, kc, dtype=torch.int64, device="cuda")
        D = torch.empty(nq, k, dtype=torch.float32, device="cuda")
        I = torch.empty(nq, k, dtype=torch.int64, device="cuda")
        ws = torch.empty(lib.wise_pqflat_topk_workspace_bytes(N, m, nq, kc), dtype=torch.uint8, device="cuda")

        def tables():
            _lib.check(lib.wise_pq_lut(q.data_ptr(), r8.codebooks.data_ptr(), nq, d, m, lut.data_ptr(), _lib.stream_ptr()), "wise_pq_lut")

        def scan_k():
            _lib.check(lib.wise_pqflat_topk(C.data_ptr(), N, m, lut.data_ptr(), nq, k, ids.data_ptr(), 0, D.data_ptr(), I.data_ptr(), ws.data_ptr(),
                                            ws.numel(), _lib.stream_ptr()), "wise_pqflat_topk")

        def scan_candidates():
            _lib.check(lib.wise_pqflat_topk(C.data_ptr(), N, m, lut.data_ptr(), nq, kc, 0, 0, cD.data_ptr(), cand.data_ptr(), ws.data_ptr(),
                                            ws.numel(), _lib.stream_ptr()), "wise_pqflat_topk")

        def refine():
            _lib.check(lib.wise_ivf_refine(rows8.data_ptr(), 8, scales8.data_ptr(), N, d, ids.data_ptr(), q.data_ptr(), nq, cand.data_ptr(), kc, k,
                                           D.data_ptr(), I.data_ptr(), _lib.stream_ptr()), "wise_ivf_refine")
        tables()
        scan_candidates()
        res = alternate({"tables": tables, f"scan_k{k}": scan_k, f"scan_k{kc}": scan_candidates, "refine": refine}, a.iters)
        out["points"][f"stages_nq{nq}"] = res
        show(f"stages nq={nq}", res)
    one = out["points"]["stages_nq1"][f"scan_k{k}"]
    one["code_bytes"] = N * m
    one["code_bytes_per_second"] = N * m / one["median"]
    one["lookups_per_second"] = N * m / one["median"]
    sq8_rate = N * d / out["points"]["nq1"]["IndexSQ8bit"]["median"]
    out["derived_floors_seconds"] = {
        "hbm": N * m / sq8_rate, "hbm_rate_bytes_per_second_of_IndexSQ8bit_in_this_run": sq8_rate,
        "lds_lookups_conflict_free": N * m / (CUS * LOOKUPS_PER_CLOCK_PER_CU * a.clock_ghz * 1e9), "assumed_clock_ghz": a.clock_ghz}
    out["hbm_bytes"] = {name: (idx.hbm_bytes() if name != "IndexFlatIP" else
                               N * (4 * d + 8) + (0 if flat._Xq is None else N * (d + 4)) + (0 if flat._Xb is None else N * d * 2))
                        for name, idx in types.items()}
    print(json.dumps({k_: out[k_] for k_ in ("hbm_bytes", "recall_at_k_vs_fp32", "derived_floors_seconds")}), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

"""numpy restatement of IndexSQfp16L2 (include/wise_hip.h: the wise_l2sq16_* entry points) the tests hold the kernels and the index to.
A test helper beside tests/sqfp16_flat_ref.py and tests/l2_flat_ref.py, whose fma32, rounded subtraction, selection and range rule it
reuses: imported by tests only, never by wise_amd/.

THE DISTANCE IS A CONTRACT (restated from the header).  Rows are binary16 (encode: numpy's float32 -> float16 cast, the bits of
wise_sq16_encode).  d % 16 == 0, 16 <= d <= 1024, C = d / 16.  Chunk c of a row is the elements 8 c .. 8 c + 7 (i = 0 .. 7) and
d / 2 + 8 c .. d / 2 + 8 c + 7 (i = 8 .. 15).  s_c = +0; for i = 0 .. 15 in order t = q[e] - float32(h[e]) (the widening is exact,
subnormals kept; ONE rounded float32 subtraction), then s_c = fma32(t, t, s_c).  Then for step = 1, 2, 4, ... < C, at once for every
c with c + step < C: s_c = s_c + s_{c + step}.  dist = s_0.  Selection: the smaller distance first, then the lower position; padding
(+3.4028235e38, -1).  A range hit is dist < radius, strictly; a query's hits come by ascending distance, ties by ascending position.

  half_norms, max_norm   what wise_l2sq16_prepare writes: half[r] in its fixed order, norms[0] = sqrt32(2 max half)
  band_terms             the terms of the batched search's eps (DESIGN.md section 4, l2_stage_kernel<_Float16, false>)
  quality_study          tests/golden/sqfp16_l2_quality.json: what the rows' rounding to binary16 costs
  band_study             tests/golden/sqfp16_l2_band.json: the collect error against eps, and the longest candidate list
"""
import numpy as np

import l2_flat_ref
from ivfsq_ref import fma32
from ivfsqfp16_ref import encode

PAD = l2_flat_ref.PAD
U32 = 2.0 ** -24          # unit roundoff of float32

__all__ = ["PAD", "encode", "chunked", "dists", "topk", "topk_pos", "range_search", "half_norms", "max_norm", "rounding_term",
           "real_dists", "band_terms", "band_study", "quality_study", "error_bound"]


def chunked(A):
    """[n, C, 16] float32: element i of chunk c of every row of A [n, d] (float16 or float32 values), in the chain's order"""
    A = np.asarray(A).astype(np.float32)
    n, d = A.shape
    assert d % 16 == 0 and 16 <= d <= 1024
    C = d // 16
    return np.ascontiguousarray(A.reshape(n, 2, C, 8).transpose(0, 2, 1, 3)).reshape(n, C, 16)


def dists(halves, Q):
    """[nq, N] float32: the contract's distance of every (query, row)."""
    halves = np.asarray(halves)
    assert halves.dtype == np.float16
    Hc, Qc = chunked(halves), chunked(np.asarray(Q, dtype=np.float32))
    n, C, _ = Hc.shape
    out = np.empty((Qc.shape[0], n), dtype=np.float32)
    for qi in range(Qc.shape[0]):
        s = np.zeros((n, C), dtype=np.float32)
        for i in range(16):
            t = Qc[qi, :, i][None, :] - Hc[:, :, i]
            assert t.dtype == np.float32
            s = fma32(t, t, s).reshape(n, C)
        step = 1
        while step < C:
            nxt = s.copy()
            nxt[:, :C - step] = s[:, :C - step] + s[:, step:]
            s = nxt
            step <<= 1
        assert s.dtype == np.float32
        out[qi] = s[:, 0]
    return out


def topk_pos(halves, Q, k, pos, ids=None, id_base=0, S=None):
    """(D [nq,k] float32 ascending, I [nq,k] int64) among the rows pos (ascending positions); S: dists(halves, Q) if already known."""
    S = dists(halves, Q) if S is None else S
    return l2_flat_ref.topk_pos(None, None, k, pos, ids=ids, id_base=id_base, S=S)


def topk(halves, Q, k, ids=None, id_base=0, S=None):
    S = dists(halves, Q) if S is None else S
    return topk_pos(halves, Q, k, np.arange(S.shape[1]), ids=ids, id_base=id_base, S=S)


def range_search(halves, Q, radius, ids=None, id_base=0, keep=None, S=None):
    """(lims [nq + 1] int64, D float32, I int64): every row with dist < float32(radius), per query by ascending distance, ties by
    ascending position; keep: bool [N], only those rows can be hits."""
    S = dists(halves, Q) if S is None else S
    return l2_flat_ref.range_search(None, None, radius, ids=ids, id_base=id_base, keep=keep, S=S)


def half_norms(halves):
    """[N] float32: half[r] of wise_l2sq16_prepare — lane l of 64 runs s = fma32(x, x, s) from +0 over the widened elements of the
    row's 16-byte pieces (8 halves) l, l + 64 in ascending order; s = s + s[lane ^ o] for o = 32, 16, 8, 4, 2, 1; the exact halving."""
    X = np.asarray(halves).astype(np.float32)
    n, d = X.shape
    pieces = d // 8
    s = np.zeros((n, 64), dtype=np.float32)
    P = X.reshape(n, pieces, 8)
    for p0 in range(0, pieces, 64):
        w = min(64, pieces - p0)
        for j in range(8):
            x = P[:, p0:p0 + w, j]
            s[:, :w] = fma32(x, x, s[:, :w]).reshape(n, w)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    assert s.dtype == np.float32
    return np.float32(0.5) * s[:, 0]


def max_norm(half):
    """float32: norms[0] of wise_l2sq16_prepare, sqrt32(2 max_r half[r]); 0 for no rows"""
    half = np.asarray(half, dtype=np.float32)
    return np.sqrt(np.float32(2.0) * (half.max() if half.size else np.float32(0.0)), dtype=np.float32)


def rounding_term(d, Q, halves):
    """[nq] float64: (d + 2) 2^-24 (|q| + max_r |h_r|)^2, the documented bound on |dist - the real-number squared distance to the
    STORED row| (l2_flat_ref.rounding_term's argument: one rounding a difference, 16 a chain, log2 C <= 6 in the fold)"""
    return l2_flat_ref.rounding_term(d, Q, np.asarray(halves).astype(np.float64))


def real_dists(halves, Q):
    """[nq, N] float64: the squared distances to the stored rows in float64"""
    return l2_flat_ref.real_dists(np.asarray(halves).astype(np.float64), Q)


# ---- the quality study (CPU only): tests/golden/sqfp16_l2_quality.json ------------------------------------------------------------------
def error_bound(X, halves, Q):
    """[nq] float64: a bound on |dist16(q, r) - dist32(q, r)| for every row r, from the data alone.  dist32 = IndexFlatL2's contract
    distance to the float32 row x_r (l2_flat_ref.dists), dist16 = this contract's distance to h_r = f16(x_r).  In real numbers
      | |q - h|^2 - |q - x|^2 | = |(x - h) . (2 q - x - h)| <= |x - h| (|q - x| + |q - h|) <= R (2 (|q| + M) + R)
    with R = max_r |x_r - h_r| and M = max_r |x_r|, and each contract distance is within (d + 2) 2^-24 (|q| + M + R)^2 of its real
    one (rounding_term).  Norms are taken in float64."""
    X = np.asarray(X, dtype=np.float64)
    H = np.asarray(halves).astype(np.float64)
    qn = np.linalg.norm(np.asarray(Q, dtype=np.float64), axis=1)
    d = X.shape[1]
    R, M = np.linalg.norm(X - H, axis=1).max(), np.linalg.norm(X, axis=1).max()
    return R * (2.0 * (qn + M) + R) + 2.0 * (d + 2) * U32 * (qn + M + R) ** 2


def quality_study(seed, cfg=None):
    """On the seeded set of ivf_l2_ref.recall_study (60,000 x 128 clustered rows times lengths log-uniform over [1, 4], queries beside
    rows): recall@k of IndexSQfp16L2 (the restatement above) against the exact float64 L2 answer over the float32 rows, the largest
    |dist16 - dist32| over every (query, row) — dist32: IndexFlatL2's contract distance —, the derived bound on it and the largest
    per-query ratio of the two.  -> dict of floats."""
    import ivf_l2_ref
    from ivfpq_refine_ref import clustered_rows_like_the_bench

    cfg = ivf_l2_ref.STUDY if cfg is None else cfg
    N, d, nlist, k, nq = cfg["rows"], cfg["dim"], cfg["nlist"], cfg["k"], cfg["queries"]
    U, _ = clustered_rows_like_the_bench(N, d, max(nlist // 2, 16), cfg["noise"], seed)
    rng = np.random.default_rng(seed + 1000)
    X = (U * np.exp(rng.uniform(0.0, np.log(cfg["spread"]), size=(N, 1)))).astype(np.float32)
    e = rng.standard_normal((nq, d))
    Q = (X[:nq] + 0.05 * np.linalg.norm(X[:nq], axis=1, keepdims=True) * e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32)
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    exact = (Q64 * Q64).sum(axis=1)[:, None] + (X64 * X64).sum(axis=1)[None, :] - 2.0 * (Q64 @ X64.T)
    pos = np.arange(N)
    If = np.stack([np.lexsort((pos, exact[q]))[:k] for q in range(nq)])
    halves = encode(X)
    S16, S32 = dists(halves, Q), l2_flat_ref.dists(X, Q)
    I16 = np.stack([np.lexsort((pos, S16[q]))[:k] for q in range(nq)])
    I32 = np.stack([np.lexsort((pos, S32[q]))[:k] for q in range(nq)])
    gap = np.abs(S16.astype(np.float64) - S32.astype(np.float64)).max(axis=1)
    bound = error_bound(X, halves, Q)
    mag = np.abs(halves.astype(np.float64))
    return {"recall": ivf_l2_ref._recall(I16, If), "recall_flat_l2": ivf_l2_ref._recall(I32, If), "max_abs_dist_gap": float(gap.max()),
            "bound": float(bound.max()), "gap_over_bound_max": float((gap / bound).max()),
            "subnormal_share": float(np.mean((mag > 0) & (mag < 2.0 ** -14)))}


# ---- the error band of the batched search (CPU only): tests/golden/sqfp16_l2_band.json --------------------------------------------------
# 40,000 rows around 64 centres times lengths log-uniform over [1, 4] (not normalised: the rows IndexSQfp16L2 is for), 64 queries
# beside rows, k = 10, a 1-in-16 sample of the rows for the threshold
STUDY = dict(rows=40000, centres=64, noise=0.35, spread=4.0, queries=64, query_noise=0.05, k=10, sample_every=16, contract_queries=4)


def band_terms(d, Q, M):
    """The terms of eps (DESIGN.md section 4, l2_stage_kernel<_Float16, false>) in float64, per query: dict of [nq] arrays.  M: the largest norm
    of a stored row.  There is no row-rounding term: the stored rows are the matrix-core operands."""
    Q = np.asarray(Q, dtype=np.float32)
    with np.errstate(over="ignore"):
        q16 = Q.astype(np.float16).astype(np.float64)
    q64 = Q.astype(np.float64)
    nq_, ne = np.linalg.norm(q64, axis=1), np.linalg.norm(q64 - q16, axis=1)
    return {"query_rounding": ne * M, "accumulation": d * 4 * U32 * nq_ * M, "half_norm": d * U32 * 0.5 * M * M * np.ones_like(nq_),
            "contract": (d + 2) * U32 * (nq_ + M) ** 2, "subnormal": np.sqrt(d) * (nq_ + M) * 2.0 ** -125 + 1e-33}


def band_study(d, seed=0, cfg=STUDY):
    """One seeded set: per term of eps the largest observed error over all (query, row) and the smallest bound over the queries
    (observed <= bound must hold query by query; the ratio recorded is the largest per-query one), the same for their sum against
    the real half-distance to the stored row, and the longest candidate list under the threshold of a 1-in-sample_every sample.
    float64 stands for the real numbers; the fp32 accumulation is numpy's float32 matrix product, not the matrix cores' (their
    order is unknown to this file).  The subnormal term has no observation of its own: it is part of the sum."""
    N, nq, k = cfg["rows"], cfg["queries"], cfg["k"]
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((cfg["centres"], d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    e = rng.standard_normal((N, d))
    X = c[rng.integers(0, cfg["centres"], size=N)] + cfg["noise"] * e / np.linalg.norm(e, axis=1, keepdims=True)
    X = X / np.linalg.norm(X, axis=1, keepdims=True) * np.exp(rng.uniform(0.0, np.log(cfg["spread"]), size=(N, 1)))
    H = encode(X.astype(np.float32))
    H32 = H.astype(np.float32)
    Q = (H32[:nq] + cfg["query_noise"] * np.linalg.norm(H32[:nq], axis=1, keepdims=True) * rng.standard_normal((nq, d)) / np.sqrt(d)).astype(np.float32)
    q16 = Q.astype(np.float16).astype(np.float32)
    H64, Q64, q1664 = H.astype(np.float64), Q.astype(np.float64), q16.astype(np.float64)
    M = float(np.linalg.norm(H64, axis=1).max())
    terms = band_terms(d, Q, M)
    half = half_norms(H)
    q2 = (Q64 * Q64).sum(axis=1)
    delta = q2[:, None] + (H64 * H64).sum(axis=1)[None, :] - 2.0 * (Q64 @ H64.T)            # the real squared distances to the stored rows
    acc32 = (q16 @ H32.T).astype(np.float64)                                                   # float32 accumulation
    obs = {"query_rounding": np.abs((Q64 - q1664) @ H64.T).max(axis=1),
           "accumulation": np.abs(acc32 - q1664 @ H64.T).max(axis=1),
           "half_norm": np.full(nq, np.abs(half.astype(np.float64) - 0.5 * (H64 * H64).sum(axis=1)).max())}
    nc = cfg["contract_queries"]                                                               # the restatement is slow: a few queries
    obs["contract"] = np.abs(dists(H, Q[:nc]).astype(np.float64) - real_dists(H, Q[:nc])).max(axis=1)
    out = {"d": d, "seed": seed, "max_row_norm": M, "max_row_norm_prepare": float(max_norm(half)), "terms": {}}
    for name, o in obs.items():
        b = terms[name][:len(o)]
        out["terms"][name] = {"observed": float(o.max()), "bound": float(b.min()), "ratio": float((o / b).max())}
    eps = sum(terms.values())
    a = half.astype(np.float64)[None, :] - acc32                                               # the approximate half-distance
    total = np.abs(a - (delta - q2[:, None]) / 2.0).max(axis=1)
    out["total"] = {"observed": float(total.max()), "bound": float(eps.min()), "ratio": float((total / eps).max())}
    t = np.sort(delta[:, ::cfg["sample_every"]], axis=1)[:, k - 1]                             # the sample's k-th distance
    listed = (a <= ((t - q2) / 2.0 + eps)[:, None])
    exact_topk = np.argsort(delta, axis=1, kind="stable")[:, :k]
    out["topk_rows_listed"] = bool(np.take_along_axis(listed, exact_topk, axis=1).all())
    out["longest_list"] = int(listed.sum(axis=1).max())
    return out


if __name__ == "__main__":      # python tests/sqfp16_l2_ref.py: recompute the two goldens
    import json
    import sys
    from pathlib import Path

    import ivf_l2_ref

    gold_dir = Path(__file__).resolve().parent / "golden"
    runs = []
    for d in (256, 1024):
        runs.append(band_study(d))
        print(json.dumps(runs[-1]), flush=True)
    gold = {"what": "sqfp16_l2_ref.band_study (numpy only, no GPU): " + json.dumps(STUDY) + "; per term of the batched search's eps the "
                    "largest observed error, the smallest bound over the queries and the largest per-query ratio; total = all terms "
                    "together against the real half-distance to the stored row; longest_list = rows a query lists under the sample's "
                    "threshold (a list holds 4096)",
            "runs": runs}
    (gold_dir / "sqfp16_l2_band.json").write_text(json.dumps(gold, indent=1) + "\n")
    if "--band-only" in sys.argv:
        sys.exit(0)
    seeds = [0, 1, 2, 3, 4]
    runs = []
    for s in seeds:
        runs.append(quality_study(s))
        print(s, json.dumps(runs[-1]), flush=True)
    gold = {"what": "sqfp16_l2_ref.quality_study (numpy restatements only, no GPU) for five seeds: " + json.dumps(ivf_l2_ref.STUDY)
                    + " (rows, dim, noise, spread, k and queries are what this study uses); recall = recall@10 of IndexSQfp16L2 against "
                      "the exact float64 L2 answer over the float32 rows; recall_flat_l2 = the same of IndexFlatL2's contract distance; "
                      "max_abs_dist_gap = the largest |dist16 - dist32| over every (query, row); bound = the largest derived bound "
                      "(sqfp16_l2_ref.error_bound); gap_over_bound_max = the largest per-query ratio; subnormal_share = stored components "
                      "with 0 < |h| < 2^-14.  Only the first seed is recomputed by tests/test_sqfp16_l2_cpu.py.",
            "seeds": seeds, "runs": runs, "recall_min": min(r["recall"] for r in runs),
            "max_abs_dist_gap": max(r["max_abs_dist_gap"] for r in runs),
            "gap_over_bound_max": max(r["gap_over_bound_max"] for r in runs)}
    (gold_dir / "sqfp16_l2_quality.json").write_text(json.dumps(gold, indent=1) + "\n")

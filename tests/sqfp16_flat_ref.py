"""numpy restatement of IndexSQfp16 (include/wise_hip.h: the wise_ipsq16_* entry points) the tests hold the kernels and the index to.
A test helper beside tests/ivfsqfp16_ref.py, whose scoring routine (row_sums: the wise_ivfsq16_scan arithmetic) it reuses: imported by
tests only.

  encode           numpy's float32 -> float16 cast: round to nearest even, subnormal halves kept, overflow to +-inf
  scores           THE CONTRACT: score(q, r) = s_0 of ivfsqfp16_ref.row_sums — chunks e(c, i), one fma32 chain of 16 per chunk, the
                   tree of adds over steps 1, 2, 4, ... — and NO bias: the value s_0 itself (a -0 stays -0)
  topk, topk_pos   selection by the kernels' key: the higher score first (-0 below +0), then the lower position;
                   (-3.4028235e38, -1) padding; ids None -> id_base + position.  topk_pos: only the listed positions compete
  range_search     every row with score > radius, strictly, per query by descending score, ties by ascending position
  error_bound      the derived bound on |score16 - score32| of the quality study (tests/test_sqfp16_flat_cpu.py)
"""
import numpy as np

from ivfsq_ref import NEG, STUDY, _recall, f32_order
from ivfsqfp16_ref import encode, row_sums

__all__ = ["NEG", "STUDY", "encode", "scores", "topk", "topk_pos", "range_search", "error_bound", "quality_study"]


def scores(halves, Q):
    """[nq, n] float32: the contract's score of every row under every query."""
    halves = np.asarray(halves, dtype=np.float16)
    Q = np.asarray(Q, dtype=np.float32)
    out = np.zeros((Q.shape[0], halves.shape[0]), dtype=np.float32)
    if halves.shape[0]:
        for q in range(Q.shape[0]):
            out[q] = row_sums(halves, Q[q])
    return out


def _select(s, pos, k, ids, id_base):
    D = np.full((k,), NEG, dtype=np.float32)
    I = np.full((k,), -1, dtype=np.int64)
    order = np.lexsort((pos, -f32_order(s)))[:k]
    D[:len(order)] = s[order]
    I[:len(order)] = pos[order] + id_base if ids is None else np.asarray(ids)[pos[order]]
    return D, I


def topk(halves, Q, k, ids=None, id_base=0, S=None):
    """(D [nq,k] float32, I [nq,k] int64) of wise_ipsq16_topk.  S: scores(halves, Q) computed before (shared between tests)."""
    S = scores(halves, Q) if S is None else S
    pos = np.arange(S.shape[1], dtype=np.int64)
    out = [_select(S[q], pos, k, ids, id_base) for q in range(S.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def topk_pos(halves, Q, k, pos, ids=None, id_base=0, S=None):
    """wise_ipsq16_topk_pos: the same over the positions pos (ascending int64) alone — the restatement restricted to those rows."""
    S = scores(halves, Q) if S is None else S
    pos = np.asarray(pos, dtype=np.int64)
    out = [_select(S[q][pos], pos, k, ids, id_base) for q in range(S.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def range_search(halves, Q, radius, ids=None, id_base=0, keep=None, S=None):
    """(lims [nq+1], D, I): every row with score > radius (and keep[row], where keep — bool [n] — is given), each query's segment
    by descending score, ties by ascending position."""
    S = scores(halves, Q) if S is None else S
    lims, Ds, Is = [0], [], []
    for q in range(S.shape[0]):
        hit = S[q] > np.float32(radius)
        if keep is not None:
            hit &= np.asarray(keep, dtype=bool)
        pos = np.flatnonzero(hit).astype(np.int64)
        order = np.lexsort((pos, -f32_order(S[q][pos])))
        pos = pos[order]
        Ds.append(S[q][pos])
        Is.append(pos + id_base if ids is None else np.asarray(ids)[pos])
        lims.append(lims[-1] + len(pos))
    return (np.asarray(lims, dtype=np.int64), np.concatenate(Ds).astype(np.float32) if Ds else np.zeros(0, np.float32),
            np.concatenate(Is).astype(np.int64) if Is else np.zeros(0, np.int64))


# ---- the quality study of tests/golden/sqfp16_flat_quality.json (CPU only) on the set of the other studies ----------------------------
U32 = 2.0 ** -24          # unit roundoff of float32


def error_bound(X, halves, Q):
    """[nq] float64: a bound on |score16(q, r) - score32(q, r)| for every row r, from the data alone.
    score32 = the float32 matrix product x_r . q (any summation order of d terms), score16 = the contract's score of h_r = f16(x_r).
      |score16 - score32| <= |q . (h_r - x_r)| + |score16 - q . h_r| + |score32 - q . x_r|
                          <= |q| max_r |x_r - h_r|                       Cauchy-Schwarz on the rounding of the rows
                           + gamma(22) |q| max_r |h_r|                   the contract's sum: 16 fma and log2(d / 16) <= 6 adds deep
                           + gamma(d) |q| max_r |x_r|                    a float32 sum of d products in any order
    with gamma(n) = n u / (1 - n u), u = 2^-24, and sum_i |q_i y_i| <= |q| |y|.  Norms are taken in float64."""
    X = np.asarray(X, dtype=np.float64)
    H = np.asarray(halves, dtype=np.float64)
    qn = np.linalg.norm(np.asarray(Q, dtype=np.float64), axis=1)
    d = X.shape[1]
    gamma = lambda n: n * U32 / (1.0 - n * U32)
    return qn * (np.linalg.norm(X - H, axis=1).max() + gamma(22) * np.linalg.norm(H, axis=1).max() + gamma(d) * np.linalg.norm(X, axis=1).max())


def quality_study(seed, cfg=STUDY):
    """On the seeded clustered rows and queries of ivfsq_ref.recall_study (60,000 x 128): recall@k of IndexSQfp16 (the restatement
    above) against float32 brute force (numpy's float32 matrix product, ties by position), the largest |score16 - score32| over every
    (query, row), the derived bound on it, and the share of stored components in the binary16 subnormal range.  -> dict of floats."""
    from ivfpq_refine_ref import clustered_rows_like_the_bench

    N, d, nlist, k, nq = cfg["rows"], cfg["dim"], cfg["nlist"], cfg["k"], cfg["queries"]
    X, _ = clustered_rows_like_the_bench(N, d, max(nlist // 2, 16), cfg["noise"], seed)
    rng = np.random.default_rng(seed + 1000)
    e = rng.standard_normal((nq, d))
    Q = X[:nq] + 0.05 * e / np.linalg.norm(e, axis=1, keepdims=True)
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    X = np.asarray(X, dtype=np.float32)
    halves = encode(X)
    S16 = scores(halves, Q)
    S32 = (Q @ X.T).astype(np.float32)
    pos = np.arange(N, dtype=np.int64)
    I16 = np.stack([np.lexsort((pos, -f32_order(S16[q])))[:k] for q in range(nq)])
    I32 = np.stack([np.lexsort((pos, -f32_order(S32[q])))[:k] for q in range(nq)])
    gap = np.abs(S16.astype(np.float64) - S32.astype(np.float64)).max(axis=1)
    bound = error_bound(X, halves, Q)
    mag = np.abs(halves.astype(np.float64))
    return {"recall": _recall(I16, I32), "max_abs_score_gap": float(gap.max()), "bound": float(bound.max()),
            "gap_over_bound_max": float((gap / bound).max()), "subnormal_share": float(np.mean((mag > 0) & (mag < 2.0 ** -14)))}


if __name__ == "__main__":      # python tests/sqfp16_flat_ref.py: recompute tests/golden/sqfp16_flat_quality.json
    import json
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent))
    seeds = [0, 1, 2, 3, 4]
    runs = []
    for s in seeds:
        runs.append(quality_study(s))
        print(s, json.dumps(runs[-1]), flush=True)
    gold = {"what": "sqfp16_flat_ref.quality_study (numpy restatements only, no GPU) for five seeds: " + json.dumps(STUDY)
                    + " (rows, dim, noise, k and queries are what this study uses); recall = recall@10 of IndexSQfp16 against float32 "
                      "brute force; max_abs_score_gap = the largest |score16 - score32| over every (query, row); bound = the largest "
                      "derived bound (sqfp16_flat_ref.error_bound); subnormal_share = stored components with 0 < |h| < 2^-14."
                      " Only the first seed is recomputed by tests/test_sqfp16_flat_cpu.py (20 s of numpy a seed); for the other four the "
                      "recorded gap is held against the recorded bound, both written by this script from the data in one run.",
            "seeds": seeds, "runs": runs, "recall_min": min(r["recall"] for r in runs),
            "max_abs_score_gap": max(r["max_abs_score_gap"] for r in runs)}
    (Path(__file__).resolve().parent / "golden" / "sqfp16_flat_quality.json").write_text(json.dumps(gold, indent=1) + "\n")

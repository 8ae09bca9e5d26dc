"""numpy restatement of IndexSQ8bit (include/wise_hip.h: the wise_ipsq8_* entry points) the tests hold the kernels and the index to.
A test helper beside tests/ivfsq_ref.py, whose codec (train, encode, decode, query) and scoring routine (row_sums: the wise_ivfsq_scan
arithmetic) it reuses: imported by tests only.

  scores           THE CONTRACT: score(q, r) = q0[q] + s_0, ONE float32 addition; W, q0 = ivfsq_ref.query, s_0 = ivfsq_ref.row_sums
  topk, topk_pos   selection by the kernels' key: the higher score first (-0 below +0), then the lower position;
                   (-3.4028235e38, -1) padding; ids None -> id_base + position.  topk_pos: only the listed positions compete
  range_search     every row with score > radius, strictly, per query by descending score, ties by ascending position
  reconstruct      ivfsq_ref.decode of the rows that carry the ids, NaN rows for ids nobody carries (the highest position wins)
  code_norm        norms[0] of wise_ipsq8_prepare
  error_bound      the derived bound on |score8 - score32| of the quality study (tests/test_sq8_flat_cpu.py)
  band_study       the batched search's band restated: the query image, eps, the thresholds of the rounds, the lists
"""
import numpy as np

from ivfsq_ref import NEG, STUDY, _recall, decode, encode, f32_order, query, row_sums, train

__all__ = ["NEG", "STUDY", "train", "encode", "decode", "query", "row_sums", "f32_order", "scores", "topk", "topk_pos", "range_search",
           "reconstruct", "code_norm", "error_bound", "quality_study", "band_study"]


def scores(codes, vmin, vdiff, Q):
    """[nq, n] float32: the contract's score of every row under every query."""
    codes = np.asarray(codes, dtype=np.uint8)
    Q = np.asarray(Q, dtype=np.float32)
    W, q0 = query(Q, vmin, vdiff)
    out = np.zeros((Q.shape[0], codes.shape[0]), dtype=np.float32)
    if codes.shape[0]:
        for q in range(Q.shape[0]):
            out[q] = np.float32(q0[q]) + row_sums(codes, W[q])
    assert out.dtype == np.float32
    return out


def _select(s, pos, k, ids, id_base):
    D = np.full((k,), NEG, dtype=np.float32)
    I = np.full((k,), -1, dtype=np.int64)
    order = np.lexsort((pos, -f32_order(s)))[:k]
    D[:len(order)] = s[order]
    I[:len(order)] = pos[order] + id_base if ids is None else np.asarray(ids)[pos[order]]
    return D, I


def topk(S, k, ids=None, id_base=0):
    """(D [nq,k] float32, I [nq,k] int64) of wise_ipsq8_topk from S = scores(codes, vmin, vdiff, Q) (shared between tests)."""
    pos = np.arange(S.shape[1], dtype=np.int64)
    out = [_select(S[q], pos, k, ids, id_base) for q in range(S.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def topk_pos(S, k, pos, ids=None, id_base=0):
    """wise_ipsq8_topk_pos: the same over the positions pos (ascending int64) alone — the restatement restricted to those rows."""
    pos = np.asarray(pos, dtype=np.int64)
    out = [_select(S[q][pos], pos, k, ids, id_base) for q in range(S.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def range_search(S, radius, ids=None, id_base=0, keep=None):
    """(lims [nq+1], D, I): every row with score > radius (and keep[row], where keep — bool [n] — is given), each query's segment
    by descending score, ties by ascending position."""
    lims, Ds, Is = [0], [], []
    for q in range(S.shape[0]):
        hit = S[q] > np.float32(radius)
        if keep is not None:
            hit &= np.asarray(keep, dtype=bool)
        pos = np.flatnonzero(hit).astype(np.int64)
        pos = pos[np.lexsort((pos, -f32_order(S[q][pos])))]
        Ds.append(S[q][pos])
        Is.append(pos + id_base if ids is None else np.asarray(ids)[pos])
        lims.append(lims[-1] + len(pos))
    return (np.asarray(lims, dtype=np.int64), np.concatenate(Ds).astype(np.float32) if Ds else np.zeros(0, np.float32),
            np.concatenate(Is).astype(np.int64) if Is else np.zeros(0, np.int64))


def reconstruct(codes, vmin, vdiff, ids, want):
    """[len(want), d] float32 of wise_ipsq8_reconstruct: ids None -> the id is the position."""
    codes = np.asarray(codes, dtype=np.uint8)
    out = np.full((len(want), codes.shape[1]), np.nan, np.float32)
    for i, w in enumerate(want):
        hit = np.flatnonzero(np.asarray(ids) == w) if ids is not None else (np.array([w]) if 0 <= w < len(codes) else np.array([], int))
        if len(hit):
            out[i] = decode(codes[hit[-1]:hit[-1] + 1], vmin, vdiff)[0]
    return out


def code_norm(codes):
    """float32: sqrtf((float)max_r sum_c codes[r, c]^2), 0 for no rows."""
    codes = np.asarray(codes, dtype=np.int64)
    return np.sqrt(np.float32((codes * codes).sum(axis=1).max())) if len(codes) else np.float32(0)


# ---- the quality study of tests/golden/sq8_flat_quality.json (CPU only) on the set of the other studies ------------------------------
U32 = 2.0 ** -24          # unit roundoff of float32


def error_bound(X, codes, vmin, vdiff, Q):
    """[nq] float64: a bound on |score8(q, r) - score32(q, r)| for every row r, from the data alone.
    score32 = the float32 matrix product x_r . q (any summation order of d terms); score8 = the contract's score of the codes; x^_r =
    the real-number decode vmin + (code + 0.5) / 255 vdiff, so that q . x^_r = q0* + sum_i w*_i code_i with the starred values the
    real-number ones of wise_sq_query.
      |score8 - score32| <= |q . (x^_r - x_r)|            <= |q| |vdiff| / 510: half a bin in every dimension (every row lies inside
                                                             the trained ranges here), Cauchy-Schwarz
                          + |score8 - q . x^_r|           <= gamma(3) |q| max_r |vdiff code_r / 255|   W's two roundings, a product's
                                                           + gamma(23) |q| max_r |vdiff code_r / 255|  16 fma, <= 6 adds, the final add
                                                           + gamma(26) |q| |vmin + vdiff / 510|        q0: 3 roundings inside a term, <= 16 + 6
                                                             adds deep, and the final add
                          + |score32 - q . x_r|           <= gamma(d) |q| max_r |x_r|
    with gamma(n) = n u / (1 - n u), u = 2^-24, and sum_i |a_i b_i| <= |a| |b|.  Norms are taken in float64."""
    X = np.asarray(X, dtype=np.float64)
    vmin, vdiff = np.asarray(vmin, dtype=np.float64), np.asarray(vdiff, dtype=np.float64)
    qn = np.linalg.norm(np.asarray(Q, dtype=np.float64), axis=1)
    d = X.shape[1]
    gamma = lambda n: n * U32 / (1.0 - n * U32)
    scaled = np.linalg.norm(np.asarray(codes, dtype=np.float64) * vdiff[None, :] / 255.0, axis=1).max()
    return qn * (np.linalg.norm(vdiff) / 510.0 + (gamma(3) + gamma(23)) * scaled + gamma(26) * np.linalg.norm(vmin + vdiff / 510.0)
                 + gamma(d) * np.linalg.norm(X, axis=1).max())


def study_set(seed, rows, dim, nq, noise=STUDY["noise"], nlist=STUDY["nlist"]):
    """(X [rows, dim] float32, Q [nq, dim] float32): the seeded clustered rows and queries of ivfsq_ref.recall_study."""
    from ivfpq_refine_ref import clustered_rows_like_the_bench

    X, _ = clustered_rows_like_the_bench(rows, dim, max(nlist // 2, 16), noise, seed)
    rng = np.random.default_rng(seed + 1000)
    e = rng.standard_normal((nq, dim))
    Q = X[:nq] + 0.05 * e / np.linalg.norm(e, axis=1, keepdims=True)
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    return np.asarray(X, dtype=np.float32), Q


def quality_study(seed, cfg=STUDY):
    """On the seeded clustered rows and queries of ivfsq_ref.recall_study (60,000 x 128), ranges trained over EVERY row (nothing
    clamps): recall@k of IndexSQ8bit (the restatement above) against float32 brute force (numpy's float32 matrix product, ties by
    position), the largest |score8 - score32| over every (query, row), the derived bound on it and their ratio.  -> dict of floats."""
    N, k, nq = cfg["rows"], cfg["k"], cfg["queries"]
    X, Q = study_set(seed, N, cfg["dim"], nq, cfg["noise"], cfg["nlist"])
    vmin, vdiff = train(X)
    codes = encode(X, vmin, vdiff)
    S8 = scores(codes, vmin, vdiff, Q)
    S32 = (Q @ X.T).astype(np.float32)
    pos = np.arange(N, dtype=np.int64)
    I8 = np.stack([np.lexsort((pos, -f32_order(S8[q])))[:k] for q in range(nq)])
    I32 = np.stack([np.lexsort((pos, -f32_order(S32[q])))[:k] for q in range(nq)])
    gap = np.abs(S8.astype(np.float64) - S32.astype(np.float64)).max(axis=1)
    bound = error_bound(X, codes, vmin, vdiff, Q)
    return {"recall": _recall(I8, I32), "max_abs_score_gap": float(gap.max()), "bound": float(bound.max()),
            "gap_over_bound_max": float((gap / bound).max())}


# ---- the band study of tests/golden/sq8_flat_band.json (CPU only): wise_ipsq8_topk_batched's thresholds restated --------------------
BAND = dict(rows=40000, dims=[256, 1024], queries=64, k=10, seed=0, cap=4096, sample=8192)


def query_image(W):
    """(e [nq] int, image [nq, d] float32 holding binary16 values, eps_over_norm [nq] float64): sq8_stage_kernel's scaling — e puts the
    largest |W| of a query into [2^14, 2^15) — the image f16(2^e W), and the band's two terms without their factor norms[0]."""
    W = np.asarray(W, dtype=np.float32)
    mx = np.abs(W).max(axis=1)
    e = np.where(mx > 0, 14 - np.floor(np.log2(np.where(mx > 0, mx, 1.0).astype(np.float64))), 0).astype(np.int64)
    scaled = np.ldexp(W.astype(np.float64), e[:, None])
    image = scaled.astype(np.float16).astype(np.float64)
    d = W.shape[1]
    eps = np.linalg.norm(scaled - image, axis=1) + d * 2.0 ** -22 * np.linalg.norm(scaled, axis=1)
    return e, image, eps


def band_study(d, cfg=BAND):
    """One dimension of the band study: the clustered rows and queries at this d, ranges over every row; per query the observed
    collect error |image . code - 2^e s_0| (the matrix-core sum in float64: its own fp32 accumulation is what the band's second term
    allows for) over the band eps, and the lists of the rounds the host plans (flat_codec_scan.h: a sample of `sample` rows, then
    growing shares, then all rows) under the thresholds 2^e ((t - q0) - 2^-21 (|t| + |q0|)) - eps.  -> dict."""
    N, nq, k, cap = cfg["rows"], cfg["queries"], cfg["k"], cfg["cap"]
    X, Q = study_set(cfg["seed"], N, d, nq)
    vmin, vdiff = train(X)
    codes = encode(X, vmin, vdiff)
    W, q0 = query(Q, vmin, vdiff)
    e, image, eps1 = query_image(W)
    eps = eps1 * float(code_norm(codes))
    C = codes.astype(np.float64)
    # the rounds, as topk_batched plans them
    full_groups = N // 32
    S0 = min(N, cfg["sample"]) & ~31
    ratio = max(cap / (4.0 * k), 4.0)
    rounds, reach = 1, S0 * ratio
    while reach < N:
        reach *= ratio
        rounds += 1
    per = (N / S0) ** (1.0 / rounds)

    def group_rows(groups, gstride):
        g = np.arange(groups, dtype=np.int64) * gstride * 32
        return (g[:, None] + np.arange(32)[None, :]).ravel()

    ratio_max, longest, missed = 0.0, 0, 0
    for q in range(nq):
        s0 = row_sums(codes, W[q])
        S = np.float32(q0[q]) + s0
        acc = C @ image[q]
        err = np.abs(acc - np.ldexp(s0.astype(np.float64), int(e[q])))
        ratio_max = max(ratio_max, float(err.max() / eps[q]))
        best = set(np.lexsort((np.arange(N), -f32_order(S)))[:k].tolist())

        def threshold(t):
            t, b = float(t), float(q0[q])
            return np.ldexp((t - b) - (abs(t) + abs(b)) * 2.0 ** -21, int(e[q])) - eps[q] * 1.0001

        rows = group_rows(S0 // 32, full_groups // (S0 // 32))
        thr = threshold(np.sort(S[rows])[-k])
        for r in range(1, rounds + 1):
            if r == rounds:
                rows = np.arange(N)
            else:
                groups = max(1, min(full_groups, int(S0 * per ** r) // 32))
                rows = group_rows(groups, full_groups // groups)
            listed = rows[acc[rows] >= thr]
            longest = max(longest, len(listed))
            if len(listed) >= k:
                thr = max(thr, threshold(np.sort(S[listed])[-k]))
        missed += len(best - set(listed.tolist()))
    return {"dim": d, "error_over_band_max": ratio_max, "longest_list": int(longest), "missed": int(missed),
            "subnormal_share_unscaled": float(np.mean((np.abs(W) > 0) & (np.abs(W) < 2.0 ** -14)))}


if __name__ == "__main__":      # python tests/sq8_flat_ref.py: recompute tests/golden/sq8_flat_quality.json and sq8_flat_band.json
    import json
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent))
    golden = Path(__file__).resolve().parent / "golden"
    seeds = [0, 1, 2, 3, 4]
    runs = []
    for s in seeds:
        runs.append(quality_study(s))
        print(s, json.dumps(runs[-1]), flush=True)
    gold = {"what": "sq8_flat_ref.quality_study (numpy restatements only, no GPU) for five seeds: " + json.dumps(STUDY)
                    + " (rows, dim, noise, k and queries are what this study uses); ranges trained over every row; recall = recall@10 of "
                      "IndexSQ8bit against float32 brute force; max_abs_score_gap = the largest |score8 - score32| over every (query, "
                      "row); bound = the largest derived bound (sq8_flat_ref.error_bound: half a bin per dimension under Cauchy-Schwarz "
                      "plus the summation terms).  Only the first seed is recomputed by tests/test_sq8_flat_cpu.py; for the other four the "
                      "recorded gap is held against the recorded bound, both written by this script from the data in one run.",
            "seeds": seeds, "runs": runs, "recall_min": min(r["recall"] for r in runs),
            "max_abs_score_gap": max(r["max_abs_score_gap"] for r in runs)}
    (golden / "sq8_flat_quality.json").write_text(json.dumps(gold, indent=1) + "\n")
    bands = []
    for d in BAND["dims"]:
        bands.append(band_study(d))
        print(json.dumps(bands[-1]), flush=True)
    gold = {"what": "sq8_flat_ref.band_study (numpy restatements only, no GPU): " + json.dumps(BAND) + "; error_over_band_max = the "
                    "largest observed collect error over the band eps of its query; longest_list = the longest candidate list of any "
                    "round, of " + str(BAND["cap"]) + " slots; missed = rows of an exact top-k that the last round did not list",
            "runs": bands}
    (golden / "sq8_flat_band.json").write_text(json.dumps(gold, indent=1) + "\n")

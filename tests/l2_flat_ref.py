"""numpy restatement of IndexFlatL2 (include/wise_hip.h: wise_l2_*) the tests hold the kernels and the index to.
A test helper beside tests/sqfp16_flat_ref.py: imported by tests only, never by wise_amd/.

THE DISTANCE IS A CONTRACT (restated from the header).  d % 16 == 0, 16 <= d <= 1024, C = d / 16.  A row is 4 C sixteen-byte pieces
of four floats; chunk c uses the pieces c, C + c, 2 C + c, 3 C + c: element i = 0 .. 15 of the chunk is
e = (i / 4) (d / 4) + 4 c + i % 4.  s_c = +0; for i = 0 .. 15 in order t = q[e] - x[e] (one rounded float32 subtraction), then
s_c = fma32(t, t, s_c).  Then for step = 1, 2, 4, ... < C, at once for every c with c + step < C: s_c = s_c + s_{c + step}.
dist = s_0.  Selection: the smaller distance first, then the lower position; padding (+3.4028235e38, -1).  A range hit is
dist < radius, strictly; a query's hits come by ascending distance, ties by ascending position.

rounding_term(d, q, X): the documented bound on |dist - the real-number squared distance|, (d + 2) 2^-24 (|q| + max |x|)^2 —
each difference carries one rounding (relative 2^-24, so its square 2 * 2^-24), the chain of a chunk 16 more and the fold
log2 C <= 6, all relative to partial sums that never exceed the distance itself, which is at most (|q| + |x|)^2.
"""
import numpy as np

from ivfsq_ref import fma32

PAD = np.float32(3.4028234663852886e38)


def chunked(A):
    """[n, C, 16] float32: element i of chunk c of every row of A [n, d], in the chain's order"""
    A = np.asarray(A, dtype=np.float32)
    n, d = A.shape
    assert d % 16 == 0 and 16 <= d <= 1024
    C = d // 16
    return np.ascontiguousarray(A.reshape(n, 4, C, 4).transpose(0, 2, 1, 3)).reshape(n, C, 16)


def dists(X, Q):
    """[nq, N] float32: the contract's distance of every (query, row)."""
    Xc, Qc = chunked(X), chunked(Q)
    n, C, _ = Xc.shape
    out = np.empty((Qc.shape[0], n), dtype=np.float32)
    for qi in range(Qc.shape[0]):
        s = np.zeros((n, C), dtype=np.float32)
        for i in range(16):
            t = Qc[qi, :, i][None, :] - Xc[:, :, i]
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


def topk_pos(X, Q, k, pos, ids=None, id_base=0, S=None):
    """(D [nq,k] float32 ascending, I [nq,k] int64) among the rows pos (ascending positions); S: dists(X, Q) if already known."""
    S = dists(X, Q) if S is None else S
    pos = np.asarray(pos, dtype=np.int64)
    nq = S.shape[0]
    D = np.full((nq, k), PAD, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        s = S[q, pos]
        order = np.lexsort((pos, s))[:k]
        D[q, :len(order)] = s[order]
        I[q, :len(order)] = ids[pos[order]] if ids is not None else pos[order] + id_base
    return D, I


def topk(X, Q, k, ids=None, id_base=0, S=None):
    return topk_pos(X, Q, k, np.arange(np.asarray(X).shape[0]), ids=ids, id_base=id_base, S=S)


def range_search(X, Q, radius, ids=None, id_base=0, keep=None, S=None):
    """(lims [nq + 1] int64, D float32, I int64): every row with dist < float32(radius), per query by ascending distance, ties by
    ascending position; keep: bool [N], only those rows can be hits."""
    S = dists(X, Q) if S is None else S
    r = np.float32(radius)
    lims, Ds, Is = [0], [], []
    for q in range(S.shape[0]):
        hit = S[q] < r
        if keep is not None:
            hit &= np.asarray(keep, dtype=bool)
        pos = np.flatnonzero(hit)
        order = np.lexsort((pos, S[q, pos]))
        pos = pos[order]
        Ds.append(S[q, pos])
        Is.append(ids[pos] if ids is not None else pos + id_base)
        lims.append(lims[-1] + len(pos))
    return (np.asarray(lims, dtype=np.int64), np.concatenate(Ds).astype(np.float32) if Ds else np.zeros(0, np.float32),
            np.concatenate(Is).astype(np.int64) if Is else np.zeros(0, np.int64))


def rounding_term(d, Q, X):
    """[nq] float64: (d + 2) 2^-24 (|q| + max_r |x_r|)^2"""
    Q, X = np.asarray(Q, dtype=np.float64), np.asarray(X, dtype=np.float64)
    xmax = np.sqrt((X * X).sum(axis=1)).max() if X.shape[0] else 0.0
    return (d + 2) * 2.0 ** -24 * (np.sqrt((Q * Q).sum(axis=1)) + xmax) ** 2


def real_dists(X, Q):
    """[nq, N] float64: the squared distances of the float32 inputs in float64"""
    X, Q = np.asarray(X, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    return ((Q[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)


# ---- the error band of the batched search (CPU only): tests/golden/flat_l2_band.json -------------------------------------------
# 40,000 unit rows around 64 centres, 128 queries beside rows, k = 10, a 1-in-16 sample of the rows for the threshold
STUDY = dict(rows=40000, centres=64, noise=0.35, queries=128, query_noise=0.05, k=10, sample_every=16, contract_queries=4)


def to_bf16(A):
    """float32 -> the float32 value of its bf16 image, round to nearest even (finite inputs)"""
    u = np.ascontiguousarray(A, dtype=np.float32).view(np.uint32)
    r = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def half_norms(X):
    """[N] float32: half[r] of wise_l2_prepare — lane l of 64 runs s = fma32(x, x, s) from +0 over the elements of the row's 16-byte
    pieces l, l + 64, ... in ascending order; s = s + s[lane ^ o] for o = 32, 16, 8, 4, 2, 1; the exact halving."""
    X = np.asarray(X, dtype=np.float32)
    n, d = X.shape
    pieces = d // 4
    s = np.zeros((n, 64), dtype=np.float32)
    P = X.reshape(n, pieces, 4)
    for p0 in range(0, pieces, 64):
        w = min(64, pieces - p0)
        for j in range(4):
            x = P[:, p0:p0 + w, j]
            s[:, :w] = fma32(x, x, s[:, :w]).reshape(n, w)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    assert s.dtype == np.float32
    return np.float32(0.5) * s[:, 0]


def band_terms(d, Q, M, Rx):
    """The terms of eps in float64, per query: dict of [nq] arrays."""
    Q = np.asarray(Q, dtype=np.float32)
    qb = to_bf16(Q).astype(np.float64)
    q64 = Q.astype(np.float64)
    nq_, ne, nb = np.linalg.norm(q64, axis=1), np.linalg.norm(q64 - qb, axis=1), np.linalg.norm(qb, axis=1)
    u = 2.0 ** -24
    return {"query_rounding": ne * M, "row_rounding": nb * Rx, "accumulation": d * 4 * u * nq_ * (M + Rx),
            "half_norm": d * u * 0.5 * M * M * np.ones_like(nq_), "contract": (d + 2) * u * (nq_ + M) ** 2}


def band_study(d, seed=0, cfg=STUDY):
    """One seeded set: per term of eps the largest observed error over all (query, row) and the smallest bound over the queries
    (observed <= bound must hold query by query; the ratio recorded is the largest per-query one), the same for their sum, and the
    longest candidate list under the threshold of a 1-in-sample_every sample.  float64 stands for the real numbers; the fp32
    accumulation is numpy's float32 matrix product, not the matrix cores' (their order is unknown to this file)."""
    N, nq, k = cfg["rows"], cfg["queries"], cfg["k"]
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((cfg["centres"], d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    e = rng.standard_normal((N, d))
    X = c[rng.integers(0, cfg["centres"], size=N)] + cfg["noise"] * e / np.linalg.norm(e, axis=1, keepdims=True)
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    Q = (X[:nq] + cfg["query_noise"] * rng.standard_normal((nq, d)) / np.sqrt(d)).astype(np.float32)
    xb, qb = to_bf16(X), to_bf16(Q)
    X64, Q64, xb64, qb64 = (a.astype(np.float64) for a in (X, Q, xb, qb))
    M = float(np.linalg.norm(X64, axis=1).max())
    Rx = float(np.linalg.norm(X64 - xb64, axis=1).max())
    terms = band_terms(d, Q, M, Rx)
    half = half_norms(X)
    q2 = (Q64 * Q64).sum(axis=1)
    delta = q2[:, None] + (X64 * X64).sum(axis=1)[None, :] - 2.0 * (Q64 @ X64.T)            # the real squared distances
    acc32 = (qb @ xb.T).astype(np.float64)                                                     # float32 accumulation
    obs = {"query_rounding": np.abs((Q64 - qb64) @ X64.T).max(axis=1),
           "row_rounding": np.abs(qb64 @ (X64 - xb64).T).max(axis=1),
           "accumulation": np.abs(acc32 - qb64 @ xb64.T).max(axis=1),
           "half_norm": np.full(nq, np.abs(half.astype(np.float64) - 0.5 * (X64 * X64).sum(axis=1)).max())}
    nc = cfg["contract_queries"]                                                               # the restatement is slow: a few queries
    obs["contract"] = np.abs(dists(X, Q[:nc]).astype(np.float64) - real_dists(X, Q[:nc])).max(axis=1)
    out = {"d": d, "seed": seed, "max_row_norm": M, "max_row_residual": Rx, "terms": {}}
    for name, bound in terms.items():
        o = obs[name]
        b = bound[:len(o)]
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


if __name__ == "__main__":      # python tests/l2_flat_ref.py: recompute tests/golden/flat_l2_band.json
    import json
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent))
    runs = []
    for d in (256, 1024):
        runs.append(band_study(d))
        print(json.dumps(runs[-1]), flush=True)
    gold = {"what": "l2_flat_ref.band_study (numpy only, no GPU): " + json.dumps(STUDY) + "; per term of the batched search's eps the "
                    "largest observed error, the smallest bound over the queries and the largest per-query ratio; total = all terms "
                    "together against the real half-distance; longest_list = rows a query lists under the sample's threshold",
            "runs": runs}
    (Path(__file__).resolve().parent / "golden" / "flat_l2_band.json").write_text(json.dumps(gold, indent=1) + "\n")

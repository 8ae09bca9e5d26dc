"""numpy restatement of the re-ranking stage of IndexIVFPQ<m>R8 / R16 (include/wise_hip.h, wise_ivf_refine) the tests hold
the kernel and the index to.  A test helper beside tests/ivfpq_ref.py: imported by tests only, never by wise_amd/.

  quantise_i8, quantise_bf16   the compact rows as wise_ip_shadow_i8 / wise_ip_shadow_bf16 are documented to build them
  dequantise                   the row a store stands for (what reconstruct_batch returns), float32
  scores, refine               float32 IN THE CONTRACT'S ORDER: acc = 0, acc = acc + q_i * x_i for i = 0 .. d-1 with the product
                               and the sum rounded separately, kind 8 then scale * acc — a loop over i on np.float32 arrays,
                               vectorised over the candidates; selection by (-score, position)
"""
import numpy as np

NEG = np.float32(-3.4028234663852886e38)


def quantise_i8(X):
    """(Xq [n,d] int8, scales [n] float32): scale = max|x_r| / 127, Xq = clip(rint(x * (127 / max|x_r|)), -127, 127), all in
    float32; a row of zeros has scale 0 and codes 0."""
    X = np.asarray(X, dtype=np.float32)
    mx = np.abs(X).max(axis=1)
    scales = (mx / np.float32(127.0)).astype(np.float32)
    inv = np.zeros_like(mx)
    np.divide(np.float32(127.0), mx, out=inv, where=mx > 0)
    q = np.clip(np.rint(X * inv[:, None]), np.float32(-127.0), np.float32(127.0))
    assert q.dtype == np.float32
    return q.astype(np.int8), scales


def quantise_bf16(X):
    """[n,d] uint16: the upper halves of the float32 bit patterns after round-to-nearest-even."""
    b = np.ascontiguousarray(X, dtype=np.float32).view(np.uint32)
    return ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def widen(rows, kind):
    """x_i of the contract as float32: the integer's value (kind 8), the bf16 bits shifted up (kind 16)."""
    if kind == 8:
        return np.asarray(rows, dtype=np.int8).astype(np.float32)
    return (np.asarray(rows, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def quantise(X, kind):
    """(rows, scales or None)"""
    return quantise_i8(X) if kind == 8 else (quantise_bf16(X), None)


def dequantise(rows, kind, scales=None):
    x = widen(rows, kind)
    return (np.asarray(scales, dtype=np.float32)[:, None] * x).astype(np.float32) if kind == 8 else x


def scores(rows, kind, scales, q):
    """[n] float32: the contract's chain for every row of `rows` against one query."""
    x = widen(rows, kind)
    q = np.asarray(q, dtype=np.float32)
    acc = np.zeros(x.shape[0], dtype=np.float32)
    for i in range(x.shape[1]):
        acc = acc + q[i] * x[:, i]                  # float32 * float32, then float32 + float32
    assert acc.dtype == np.float32
    return np.asarray(scales, dtype=np.float32) * acc if kind == 8 else acc


def refine(rows, kind, scales, ids, Q, cand_pos, k):
    """(D [nq,k] float32, I [nq,k] int64): candidates outside [0, N) are skipped, results by (-score, position),
    (-3.4028235e38, -1) padding."""
    N = rows.shape[0]
    nq = Q.shape[0]
    D = np.full((nq, k), NEG, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        pos = np.asarray(cand_pos[q], dtype=np.int64)
        pos = pos[(pos >= 0) & (pos < N)]
        if not len(pos):
            continue
        s = scores(rows[pos], kind, None if scales is None else scales[pos], Q[q])
        order = np.lexsort((pos, -s.astype(np.float64)))[:k]
        D[q, :len(order)] = s[order]
        I[q, :len(order)] = pos[order] if ids is None else ids[pos[order]]
    return D, I


def clustered_rows_like_the_bench(n, d, centres, noise, seed):
    """The bench tool's data recipe (tools/ivfpq_bench.py) on the host: unit centres, a unit noise direction scaled by `noise`,
    re-normalised.  -> (rows [n,d] float32, centres [centres,d] float32)."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    e = rng.standard_normal((n, d))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    x = c[rng.integers(0, centres, n)] + noise * e
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), c.astype(np.float32)


# ---- the recall study of tests/golden/ivfpq_refine_quality.json (CPU only) ------------------------------------------------
STUDY = dict(rows=60000, dim=128, m=16, nlist=244, noise=0.35, nprobe=32, k=10, queries=64, train_rows=16384, niter=5,
             k_factors=(5, 10, 20, 50, 100))


def _recall(I, If):
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / len(b) for a, b in zip(I, If)]))


def recall_study(seed, cfg=STUDY):
    """recall@k against the float64 flat answer on one seeded clustered set: of the PQ scan alone, after re-ranking its
    k * k_factor best positions by each store, and the ceilings (every probed row re-ranked by the int8 rows, the bf16 rows and
    the fp32 rows).  Everything by the restatements (ivfpq_ref and this file).  -> dict of floats / per-k_factor dicts."""
    import ivfpq_ref

    N, d, m, nlist, k, nq = cfg["rows"], cfg["dim"], cfg["m"], cfg["nlist"], cfg["k"], cfg["queries"]
    X, _ = clustered_rows_like_the_bench(N, d, max(nlist // 2, 16), cfg["noise"], seed)
    rng = np.random.default_rng(seed + 1000)
    e = rng.standard_normal((nq, d))
    Q = X[:nq] + 0.05 * e / np.linalg.norm(e, axis=1, keepdims=True)
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    c = ivfpq_ref.spherical_kmeans(X, nlist, 1234)
    a = (X @ c.T).argmax(axis=1)
    order = np.argsort(a, kind="stable")
    X, a = X[order], a[order]                                  # list order: a position is a row number from here on
    list_off = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=nlist))]).astype(np.int64)
    resid = X - c[a]
    tr = np.sort(np.random.default_rng(seed).permutation(N)[:cfg["train_rows"]])
    cb = ivfpq_ref.train(resid[tr], m, niter=cfg["niter"]).astype(np.float32)
    codes = np.concatenate([ivfpq_ref.encode(resid[s:s + 8192], cb) for s in range(0, N, 8192)])
    coarse = Q.astype(np.float64) @ c.astype(np.float64).T
    probes = np.argsort(-coarse, axis=1, kind="stable")[:, :cfg["nprobe"]].astype(np.int64)
    bias = np.take_along_axis(coarse, probes, axis=1).astype(np.float32)
    kc = k * max(cfg["k_factors"])
    _, cand = ivfpq_ref.scan(codes, list_off, None, ivfpq_ref.lut(Q, cb).astype(np.float32), probes, bias, kc)
    exact = X.astype(np.float64) @ Q.astype(np.float64).T      # [N, nq]
    If = np.stack([np.lexsort((np.arange(N), -exact[:, q]))[:k] for q in range(nq)])
    probed = [np.concatenate([np.arange(list_off[l], list_off[l + 1]) for l in probes[q]]) for q in range(nq)]
    width = max(len(p) for p in probed)
    every = np.full((nq, width), -1, dtype=np.int64)
    for q in range(nq):
        every[q, :len(probed[q])] = probed[q]
    out = {"pq_alone": _recall(cand[:, :k], If)}
    for kind in (8, 16):
        rows, scales = quantise(X, kind)
        out[f"r{kind}"] = {str(f): _recall(refine(rows, kind, scales, None, Q, cand[:, :k * f], k)[1], If) for f in cfg["k_factors"]}
        out[f"ceiling_r{kind}"] = _recall(refine(rows, kind, scales, None, Q, every, k)[1], If)
    out["ceiling_fp32"] = _recall(np.stack([probed[q][np.lexsort((probed[q], -exact[probed[q], q]))[:k]] for q in range(nq)]), If)
    return out


def study_summary(runs, at="50"):
    """What the seeded test holds one more seed to: per store the smallest gain over the PQ scan alone at k_factor `at` that the
    runs show, and the spread (max - min) of that gain."""
    s = {}
    for kind in (8, 16):
        gains = [r[f"r{kind}"][at] - r["pq_alone"] for r in runs]
        s[f"gain_min_r{kind}"], s[f"gain_spread_r{kind}"] = min(gains), max(gains) - min(gains)
    return s


if __name__ == "__main__":      # python tests/ivfpq_refine_ref.py: recompute tests/golden/ivfpq_refine_quality.json
    import json
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent))
    seeds = [0, 1, 2, 3, 4]
    runs = []
    for s in seeds:
        runs.append(recall_study(s))
        print(s, json.dumps(runs[-1]), flush=True)
    gold = {"what": "ivfpq_refine_ref.recall_study (numpy restatements only, no GPU) for five seeds: " + json.dumps(STUDY)
                    + "; recall@10 against the float64 flat answer; gains are taken at k_factor 50",
            "seeds": seeds, "runs": runs, **study_summary(runs)}
    (Path(__file__).resolve().parent / "golden" / "ivfpq_refine_quality.json").write_text(json.dumps(gold, indent=1) + "\n")

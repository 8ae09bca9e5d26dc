"""numpy restatement of IndexIVFSQfp16 (include/wise_hip.h: wise_sq16_*, wise_ivfsq16_scan) the tests hold the kernels and the index to.
A test helper beside tests/ivfsq_ref.py, whose fma32, f32_order and study set-up it reuses: imported by tests only.

  encode                  numpy's float32 -> float16 cast: round to nearest even, subnormal halves kept, overflow to +-inf
  decode, decode_rows     c_l + (float32)h, one float32 addition
  chunks                  THE CHUNKS OF A ROW: with C = d / 16, chunk c holds elements 8 c .. 8 c + 7 (i = 0 .. 7) and
                          d / 2 + 8 c .. d / 2 + 8 c + 7 (i = 8 .. 15) — the row's 16-byte pieces c and c + C
  row_sums, scan          THE SCAN'S ORDER: s_c = +0, s_c = fma32(q[e(c, i)], h[e(c, i)], s_c) for i = 0 .. 15 (a binary16 value
                          times a float32 one is exact in float64: 11 + 24 bits, so ivfsq_ref.fma32 applies unchanged); then for
                          step = 1, 2, 4, ... < C, at once for every c with c + step < C, s_c = s_c + s_{c + step};
                          score = bias + s_0.  Selection by the kernels' key: the higher score first (-0 below +0), then the lower
                          position
"""
import numpy as np

from ivfsq_ref import NEG, STUDY, _recall, f32_order, fma32, list_of_rows


def encode(resid):
    """[n,d] float16 of the float32 residuals."""
    with np.errstate(over="ignore"):
        return np.asarray(resid, dtype=np.float32).astype(np.float16)


def decode(halves, dtype=np.float32):
    """[n,d]: the residual the halves stand for."""
    return np.asarray(halves, dtype=np.float16).astype(dtype)


def decode_rows(halves, list_off, centroids, dtype=np.float32):
    """[n,d]: c_l + decode(halves), what reconstruct_batch returns for the rows in list order."""
    return np.asarray(centroids, dtype=dtype)[list_of_rows(list_off)] + decode(halves, dtype)


def chunks(x):
    """[n, d] -> [n, C, 16]: element i of chunk c in the contract's order."""
    n, d = x.shape
    C = d // 16
    return np.concatenate([x[:, :d // 2].reshape(n, C, 8), x[:, d // 2:].reshape(n, C, 8)], axis=2)


def row_sums(halves, q):
    """[n] float32: s_0 of every row of halves [n,d] under the query q [d], in the scan's order."""
    halves = np.asarray(halves, dtype=np.float16)
    n, d = halves.shape
    C = d // 16
    x = chunks(halves.astype(np.float32))
    wc = chunks(np.asarray(q, dtype=np.float32).reshape(1, d))
    s = np.zeros((n, C), dtype=np.float32)
    for i in range(16):
        s = fma32(np.broadcast_to(wc[:, :, i], (n, C)), x[:, :, i], s).reshape(n, C)
    step = 1
    while step < C:
        nxt = s.copy()
        nxt[:, :C - step] = s[:, :C - step] + s[:, step:]
        s = nxt
        step <<= 1
    assert s.dtype == np.float32
    return s[:, 0].copy()


def scores(halves, list_off, Q, probes, bias, keep=None):
    """Per query (pos [m] int64, s [m] float32): every candidate row of the probed lists in probe order, then by position, with the
    scan's score.  probes < 0 or >= nlist and empty lists are skipped; a list named twice is listed twice."""
    nlist = len(list_off) - 1
    out = []
    for q in range(probes.shape[0]):
        pos, base = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.float32)]
        for p, l in enumerate(probes[q]):
            if l < 0 or l >= nlist or list_off[l + 1] == list_off[l]:
                continue
            r = np.arange(list_off[l], list_off[l + 1], dtype=np.int64)
            pos.append(r)
            base.append(np.full(len(r), np.float32(bias[q, p]), dtype=np.float32))
        pos, base = np.concatenate(pos), np.concatenate(base)
        if keep is not None:
            sel = np.asarray(keep, dtype=bool)[pos]
            pos, base = pos[sel], base[sel]
        s = base + row_sums(halves[pos], Q[q]) if len(pos) else base
        assert s.dtype == np.float32
        out.append((pos, s))
    return out


def scan(halves, list_off, ids, Q, probes, bias, k, keep=None):
    """(D [nq,k] float32, I [nq,k] int64) of wise_ivfsq16_scan (keep: bool [N], wise_ivfsq16_scan_sel): (-3.4028235e38, -1)
    padding; ids None -> positions."""
    nq = probes.shape[0]
    D = np.full((nq, k), NEG, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for q, (pos, s) in enumerate(scores(halves, list_off, Q, probes, bias, keep)):
        order = np.lexsort((pos, -f32_order(s)))[:k]
        D[q, :len(order)] = s[order]
        I[q, :len(order)] = pos[order] if ids is None else ids[pos[order]]
    return D, I


# ---- the recall study of tests/golden/ivfsqfp16_quality.json (CPU only): the set of ivfsq_ref.recall_study -----------------------
def recall_study(seed, cfg=STUDY):
    """recall@k against the float64 flat answer on the seeded clustered set of ivfsq_ref.recall_study (same rows, queries, centroids,
    probes and bias): of IndexIVFSQfp16 by the restatement above and of IVFFlat (exact scores of the probed rows) at the same nprobe;
    the mean reconstruction error |x - x^| (L2, the rows are unit vectors), the share of stored components in the binary16 subnormal
    range and the largest residual component.  -> dict of floats."""
    import ivfpq_ref
    from ivfpq_refine_ref import clustered_rows_like_the_bench

    N, d, nlist, k, nq = cfg["rows"], cfg["dim"], cfg["nlist"], cfg["k"], cfg["queries"]
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
    resid = (X - c[a]).astype(np.float32)
    halves = encode(resid)
    coarse = Q.astype(np.float64) @ c.astype(np.float64).T
    probes = np.argsort(-coarse, axis=1, kind="stable")[:, :cfg["nprobe"]].astype(np.int64)
    bias = np.take_along_axis(coarse, probes, axis=1).astype(np.float32)
    _, I = scan(halves, list_off, None, Q, probes, bias, k)
    exact = X.astype(np.float64) @ Q.astype(np.float64).T      # [N, nq]
    If = np.stack([np.lexsort((np.arange(N), -exact[:, q]))[:k] for q in range(nq)])
    probed = [np.concatenate([np.arange(list_off[l], list_off[l + 1]) for l in probes[q]]) for q in range(nq)]
    Iflat = np.stack([probed[q][np.lexsort((probed[q], -exact[probed[q], q]))[:k]] for q in range(nq)])
    err = np.linalg.norm(X.astype(np.float64) - decode_rows(halves, list_off, c, np.float64), axis=1)
    mag = np.abs(halves.astype(np.float64))
    return {"sqfp16": _recall(I, If), "ivfflat": _recall(Iflat, If), "reconstruction_error": float(err.mean()),
            "subnormal_share": float(np.mean((mag > 0) & (mag < 2.0 ** -14))), "max_abs_residual": float(np.abs(resid).max())}


if __name__ == "__main__":      # python tests/ivfsqfp16_ref.py: recompute tests/golden/ivfsqfp16_quality.json
    import json
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent))
    seeds = [0, 1, 2, 3, 4]
    runs = []
    for s in seeds:
        runs.append(recall_study(s))
        print(s, json.dumps(runs[-1]), flush=True)
    gold = {"what": "ivfsqfp16_ref.recall_study (numpy restatements only, no GPU) for five seeds: " + json.dumps(STUDY)
                    + "; recall@10 against the float64 flat answer of IndexIVFSQfp16 and of IVFFlat at the same nprobe; "
                      "reconstruction_error = mean |x - decoded x| over the unit rows; subnormal_share = stored components with "
                      "0 < |h| < 2^-14",
            "seeds": seeds, "runs": runs,
            "sqfp16_min": min(r["sqfp16"] for r in runs), "ivfflat_min": min(r["ivfflat"] for r in runs),
            "gap_max": max(r["ivfflat"] - r["sqfp16"] for r in runs)}
    (Path(__file__).resolve().parent / "golden" / "ivfsqfp16_quality.json").write_text(json.dumps(gold, indent=1) + "\n")

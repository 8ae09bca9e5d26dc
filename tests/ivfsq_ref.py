"""numpy restatement of IndexIVFSQ8 (include/wise_hip.h: wise_sq_*, wise_ivfsq_scan) the tests hold the kernels and the index to.
A test helper beside tests/ivfpq_ref.py: imported by tests only, never by wise_amd/.

  train, decode           float32, every operation rounded on its own, as the header fixes them (decode is faiss's Codec8bit)
  encode                  the same formula with every operation in float64: the bin a value really falls into
  query                   W and q0 of wise_sq_query: q0's lanes, the order inside a lane, the butterfly
  fma32                   the float32 fused multiply-add, exact: the product and the sum in float64 with the sum's rounding error
                          recovered (TwoSum) and folded in by rounding to odd, so that the final rounding to float32 sees the
                          infinitely precise value
  row_sums, scan          THE SCAN'S ORDER: chunk c of a row (16 dimensions, one lane of the kernel) runs s_c = +0,
                          s_c = fma32(w[16 c + i], code[16 c + i], s_c) for i = 0 .. 15; then for step = 1, 2, 4, ... < C = d / 16,
                          at once for every c with c + step < C, s_c = s_c + s_{c + step}; score = (bias + q0) + s_0.
                          Selection by the kernels' key: the higher score first (-0 below +0), then the lower position
"""
import numpy as np

NEG = np.float32(-3.4028234663852886e38)
INV255 = np.float32(1.0) / np.float32(255.0)
HALF255 = np.float32(0.5) / np.float32(255.0)


def train(resid):
    """(vmin [d], vdiff [d]) float32: faiss RS_minmax with argument 0."""
    resid = np.asarray(resid, dtype=np.float32)
    vmin = resid.min(axis=0)
    return vmin, (resid.max(axis=0) - vmin).astype(np.float32)


def encode(resid, vmin, vdiff):
    """[n,d] uint8: clamp(floor((r - vmin) * (255 / vdiff)), 0, 255), inv = 0 where vdiff == 0; the float32 inputs widened, every
    operation in float64 (as wise_sq_encode)."""
    resid, vmin, vdiff = (np.asarray(np.asarray(a, dtype=np.float32), dtype=np.float64) for a in (resid, vmin, vdiff))
    inv = np.zeros_like(vdiff)
    np.divide(255.0, vdiff, out=inv, where=vdiff != 0)
    t = np.floor((resid - vmin[None, :]) * inv[None, :])
    assert t.dtype == np.float64
    return np.clip(t, 0.0, 255.0).astype(np.uint8)


def decode(codes, vmin, vdiff, dtype=np.float32):
    """[n,d]: vmin + ((code + 0.5) / 255) * vdiff — the residual a code stands for (add the list's centroid for the row).
    dtype float64: the same formula without float32 roundings."""
    f = np.dtype(dtype).type
    xi = (np.asarray(codes).astype(dtype) + f(0.5)) / f(255.0)
    return np.asarray(vmin, dtype=dtype)[None, :] + xi * np.asarray(vdiff, dtype=dtype)[None, :]


def list_of_rows(list_off):
    return np.repeat(np.arange(len(list_off) - 1), np.diff(list_off))


def decode_rows(codes, list_off, centroids, vmin, vdiff, dtype=np.float32):
    """[n,d]: c_l + decode(codes), what reconstruct_batch returns for the rows in list order."""
    return np.asarray(centroids, dtype=dtype)[list_of_rows(list_off)] + decode(codes, vmin, vdiff, dtype)


def query(Q, vmin, vdiff):
    """(W [nq,d], q0 [nq]) float32 as wise_sq_query: W = (q * vdiff) * (1 / 255); q0: lane l of 64 adds q_i * (vmin[i] + vdiff[i] *
    (0.5 / 255)) over i = l, l + 64, ... from +0, then v = v + v[lane ^ o] for o = 32, 16, 8, 4, 2, 1."""
    Q, vmin, vdiff = (np.asarray(a, dtype=np.float32) for a in (Q, vmin, vdiff))
    nq, d = Q.shape
    W = (Q * vdiff[None, :]) * INV255
    t = vmin + vdiff * HALF255
    p = Q * t[None, :]
    assert W.dtype == np.float32 and p.dtype == np.float32
    acc = np.zeros((nq, 64), dtype=np.float32)
    for i0 in range(0, d, 64):
        w = min(64, d - i0)
        acc[:, :w] = acc[:, :w] + p[:, i0:i0 + w]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    return W, acc[:, 0].copy()


def fma32(a, b, c):
    """round_to_float32(a * b + c) with one rounding, elementwise on float32 arrays."""
    p = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)          # 24 + 24 bits: exact
    c = np.asarray(c, dtype=np.float64)
    t = p + c
    bb = t - p
    err = (p - (t - bb)) + (c - bb)                                                # TwoSum: p + c == t + err exactly
    t = np.array(t, dtype=np.float64, ndmin=1)
    err = np.broadcast_to(err, t.shape)
    fix = (err != 0) & ((t.view(np.int64) & 1) == 0)                               # round to odd: an inexact even t moves towards the truth
    t[fix] = np.nextafter(t[fix], np.where(err[fix] > 0, np.inf, -np.inf))
    return t.astype(np.float32)


def row_sums(codes, w):
    """[n] float32: s_0 of every row of codes [n,d] under the weight row w [d], in the scan's order."""
    codes = np.asarray(codes, dtype=np.uint8)
    n, d = codes.shape
    C = d // 16
    x = codes.astype(np.float32).reshape(n, C, 16)
    wc = np.asarray(w, dtype=np.float32).reshape(1, C, 16)
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


def f32_order(s):
    """The scan's sortable key of a float32 score (larger = better)."""
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)
    return np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000)).astype(np.int64)


def scan(codes, list_off, ids, W, q0, probes, bias, k, keep=None):
    """(D [nq,k] float32, I [nq,k] int64) of wise_ivfsq_scan (keep: bool [N], wise_ivfsq_scan_sel): probes < 0 or >= nlist are
    skipped, (-3.4028235e38, -1) padding; ids None -> positions."""
    nq = probes.shape[0]
    nlist = len(list_off) - 1
    D = np.full((nq, k), NEG, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        pos, base = [], []
        for p, l in enumerate(probes[q]):
            if l < 0 or l >= nlist or list_off[l + 1] == list_off[l]:
                continue
            r = np.arange(list_off[l], list_off[l + 1], dtype=np.int64)
            pos.append(r)
            base.append(np.full(len(r), np.float32(bias[q, p]) + np.float32(q0[q]), dtype=np.float32))
        if not pos:
            continue
        pos, base = np.concatenate(pos), np.concatenate(base)
        if keep is not None:
            sel = np.asarray(keep, dtype=bool)[pos]
            pos, base = pos[sel], base[sel]
            if not len(pos):
                continue
        s = base + row_sums(codes[pos], W[q])
        assert s.dtype == np.float32
        order = np.lexsort((pos, -f32_order(s)))[:k]
        D[q, :len(order)] = s[order]
        I[q, :len(order)] = pos[order] if ids is None else ids[pos[order]]
    return D, I


# ---- the recall study of tests/golden/ivfsq_quality.json (CPU only) ------------------------------------------------------------
# the set of tests/golden/ivfpq_refine_quality.json (ivfpq_refine_ref.STUDY): same rows, queries, centroids, nprobe and k
STUDY = dict(rows=60000, dim=128, nlist=244, noise=0.35, nprobe=32, k=10, queries=64, train_rows=16384)


def _recall(I, If):
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / len(b) for a, b in zip(I, If)]))


def recall_study(seed, cfg=STUDY):
    """recall@k against the float64 flat answer on one seeded clustered set: of IndexIVFSQ8 by the restatement above and of
    IVFFlat (exact scores of the probed rows) at the same nprobe; the mean reconstruction error |x - x^| (L2, the rows are unit
    vectors) and the mean range per dimension.  -> dict of floats."""
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
    resid = X - c[a]
    tr = np.sort(np.random.default_rng(seed).permutation(N)[:cfg["train_rows"]])
    vmin, vdiff = train(resid[tr])
    codes = encode(resid, vmin, vdiff)
    coarse = Q.astype(np.float64) @ c.astype(np.float64).T
    probes = np.argsort(-coarse, axis=1, kind="stable")[:, :cfg["nprobe"]].astype(np.int64)
    bias = np.take_along_axis(coarse, probes, axis=1).astype(np.float32)
    W, q0 = query(Q, vmin, vdiff)
    _, I = scan(codes, list_off, None, W, q0, probes, bias, k)
    exact = X.astype(np.float64) @ Q.astype(np.float64).T      # [N, nq]
    If = np.stack([np.lexsort((np.arange(N), -exact[:, q]))[:k] for q in range(nq)])
    probed = [np.concatenate([np.arange(list_off[l], list_off[l + 1]) for l in probes[q]]) for q in range(nq)]
    Iflat = np.stack([probed[q][np.lexsort((probed[q], -exact[probed[q], q]))[:k]] for q in range(nq)])
    err = np.linalg.norm(X.astype(np.float64) - decode_rows(codes, list_off, c, vmin, vdiff, np.float64), axis=1)
    return {"sq8": _recall(I, If), "ivfflat": _recall(Iflat, If), "reconstruction_error": float(err.mean()),
            "mean_vdiff": float(vdiff.astype(np.float64).mean())}


if __name__ == "__main__":      # python tests/ivfsq_ref.py: recompute tests/golden/ivfsq_quality.json
    import json
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent))
    seeds = [0, 1, 2, 3, 4]
    runs = []
    for s in seeds:
        runs.append(recall_study(s))
        print(s, json.dumps(runs[-1]), flush=True)
    gold = {"what": "ivfsq_ref.recall_study (numpy restatements only, no GPU) for five seeds: " + json.dumps(STUDY)
                    + "; recall@10 against the float64 flat answer of IndexIVFSQ8 and of IVFFlat at the same nprobe; "
                      "reconstruction_error = mean |x - decoded x| over the unit rows",
            "seeds": seeds, "runs": runs,
            "sq8_min": min(r["sq8"] for r in runs), "ivfflat_min": min(r["ivfflat"] for r in runs),
            "gap_max": max(r["ivfflat"] - r["sq8"] for r in runs)}
    (Path(__file__).resolve().parent / "golden" / "ivfsq_quality.json").write_text(json.dumps(gold, indent=1) + "\n")

"""numpy float64 restatement of the IndexIVFOPQ pieces (a learned rotation in front of tests/ivfpq_ref.py's product quantizer)
the tests hold the GPU trainer and kernels to.  A test helper: imported by tests and tools only, never by wise_amd/.

  rotate, correlation, procrustes    y = R x;  M = sum_i cw_i x_i^T;  R = U V^T from M = U S V^T (the orthonormal R that minimises
                                     sum_i ||R x_i - cw_i||^2)
  train                              the trainer's iteration (wise_amd/index/ivf_pq.py, train_rotation): from R = I, opq_niter
                                     times {rotate, fit, encode, M, R}, then one more rotation and fit; the first fit is
                                     ivfpq_ref.train from the first 256 rotated rows, the later ones opq_niter_pq Lloyd steps
  study_data                         the seeded data of the CPU study and of tests/golden/ivfopq_quality.json
"""
import numpy as np

import ivfpq_ref

KSUB = ivfpq_ref.KSUB


def sub_scores(resid, codebooks):
    """ivfpq_ref.sub_scores as one batched matrix product (the trainer calls it a few hundred times)."""
    m, _, dsub = codebooks.shape
    r = np.asarray(resid, dtype=np.float64).reshape(resid.shape[0], m, dsub).transpose(1, 0, 2)
    cb = np.asarray(codebooks, dtype=np.float64)
    return (np.matmul(r, cb.transpose(0, 2, 1)) - 0.5 * (cb * cb).sum(axis=2)[:, None, :]).transpose(1, 0, 2)


def encode(resid, codebooks):
    return sub_scores(resid, codebooks).argmax(axis=2).astype(np.uint8)


def rotate(x, R):
    """[n, d] float64: row i = R x_i."""
    return np.asarray(x, dtype=np.float64) @ np.asarray(R, dtype=np.float64).T


def codewords(codes, codebooks):
    """[n, d] float64: concat_j cb[j][code_j]."""
    cb = np.asarray(codebooks, dtype=np.float64)
    return np.concatenate([cb[j, codes[:, j]] for j in range(cb.shape[0])], axis=1)


def correlation(codes, codebooks, x):
    """M [d, d] float64 = sum_i cw_i x_i^T (x: the UNROTATED rows)."""
    return codewords(codes, codebooks).T @ np.asarray(x, dtype=np.float64)


def procrustes(M):
    """The orthonormal R = U V^T of M = U S V^T: argmax_R trace(R M^T) = argmin_R sum_i ||R x_i - cw_i||^2."""
    u, _, vt = np.linalg.svd(np.asarray(M, dtype=np.float64))
    return u @ vt


def distortion(resid, R, codebooks):
    """Mean squared error of the rotated residuals under their nearest codewords (float64)."""
    xr = rotate(resid, R)
    m, _, dsub = codebooks.shape
    s = sub_scores(xr, codebooks).max(axis=2)
    return float(((xr * xr).sum(axis=1) - 2.0 * s.sum(axis=1)).mean())


def _lloyd(xr, cb, steps):
    for _ in range(steps):
        cb, _ = ivfpq_ref.lloyd_update(xr, encode(xr, cb), cb)
    return cb


def train(resid, m, niter=10, opq_niter=50, opq_niter_pq=4):
    """-> (R [d,d], codebooks [m,256,dsub], distortions): distortions[t] is the distortion right after the fit of outer iteration
    t (t = 0: plain PQ, R = I), distortions[opq_niter] the final one."""
    resid = np.asarray(resid, dtype=np.float64)
    d = resid.shape[1]
    R, cb, hist = np.eye(d), None, []
    for _ in range(max(int(opq_niter), 1)):
        xr = rotate(resid, R)
        cb = _lloyd(xr, np.asarray(ivfpq_ref.initial_codebooks(xr, m), dtype=np.float64), niter) if cb is None else _lloyd(xr, cb, opq_niter_pq)
        hist.append(distortion(resid, R, cb))
        R = procrustes(correlation(encode(xr, cb), cb, resid))
    cb = _lloyd(rotate(resid, R), cb, opq_niter_pq)
    hist.append(distortion(resid, R, cb))
    return R, cb, hist


# ---------------------------------------------------------------------------------------------------------------------
# the CPU study's data (tests/golden/ivfopq_quality.json; tools/make_golden_ivfopq_quality.py)
STUDY = dict(n=20000, d=64, centres=64, nlist=64, m=8, noise=0.6, seed=41, nq=200, nprobe=16, k=10, kmeans_seed=1234)


def decaying_spectrum_rows(n, d, centres, noise, seed, mixed=True):
    """n seeded unit rows around `centres` unit centres whose offsets from the centre have a decaying spectrum: coordinate i of
    the offset has deviation proportional to 1 / sqrt(1 + i) (scaled so that the offset's expected squared length is noise^2),
    and — mixed — the offsets are then turned by a seeded random orthogonal matrix, so that the spectrum's axes are not the
    product quantizer's.  Rows are re-normalised."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    s = 1.0 / np.sqrt(1.0 + np.arange(d))
    s *= noise / np.sqrt((s * s).sum())
    off = rng.standard_normal((n, d)) * s
    if mixed:
        q, r = np.linalg.qr(rng.standard_normal((d, d)))
        off = off @ (q * np.sign(np.diag(r))).T
    x = c[rng.integers(0, centres, n)] + off
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def study_data():
    """(X [n,d] fp32, Q [nq,d] fp32, centroids [nlist,d] fp32) of the study: mixed-spectrum rows, queries = seeded rows of X
    nudged by 5 % noise, the coarse quantizer of ivfpq_ref.spherical_kmeans."""
    p = STUDY
    X = decaying_spectrum_rows(p["n"], p["d"], p["centres"], p["noise"], p["seed"])
    rng = np.random.default_rng(p["seed"] + 1)
    Q = X[rng.permutation(p["n"])[:p["nq"]]] + 0.05 * rng.standard_normal((p["nq"], p["d"])).astype(np.float32) / np.sqrt(p["d"])
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    return X, Q, ivfpq_ref.spherical_kmeans(X, p["nlist"], p["kmeans_seed"])


def residuals(X, centroids):
    """(assign [n], residuals [n,d] fp32) under the nearest centroid by inner product."""
    a = (X @ centroids.T).argmax(axis=1)
    return a, (X - centroids[a]).astype(np.float32)


def recall_at_k(X, Q, centroids, R, codebooks, nprobe, k):
    """recall@k against the flat answer of an index built by the restatement: rows grouped by list, codes from the rotated
    residuals, ivfpq_ref.scan over tables built from the rotated queries.  R None: plain PQ."""
    from oracle import ip_topk_ref

    a, resid = residuals(X, centroids)
    order = np.argsort(a, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=centroids.shape[0]))]).astype(np.int64)
    R = np.eye(X.shape[1]) if R is None else R
    cb = np.asarray(codebooks, dtype=np.float32)
    codes = encode(rotate(resid[order], R), cb)
    coarse = Q.astype(np.float64) @ centroids.astype(np.float64).T
    probes = np.argsort(-coarse, axis=1, kind="stable")[:, :nprobe].astype(np.int64)
    bias = np.take_along_axis(coarse, probes, axis=1).astype(np.float32)
    lut = ivfpq_ref.lut(rotate(Q, R).astype(np.float32), cb).astype(np.float32)
    _, I = ivfpq_ref.scan(codes, off, order.astype(np.int64), lut, probes, bias, k)
    _, If = ip_topk_ref.ip_topk(X, Q, k)
    return float(np.mean([len(set(I[q]) & set(If[q])) / k for q in range(Q.shape[0])]))

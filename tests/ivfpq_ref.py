"""numpy restatement of the IndexIVFPQ pieces (8-bit codes, by_residual, inner product) the GPU tests hold the kernels to.
A test helper: imported by tests only, never by wise_amd/.

  encode, lloyd_update, lut, train   float64
  scan                               float32 IN THE CONTRACT'S ORDER (include/wise_hip.h, wise_ivfpq_scan): acc = bias, then
                                     acc += lut[j][code_j] for j = 0 .. m-1 — a loop over j on np.float32 arrays, vectorised
                                     over rows; ordered by (-score, position)
"""
import numpy as np

KSUB = 256
NEG = np.float32(-3.4028234663852886e38)
MAX_TRAIN_ROWS = 65536


def sub_scores(resid, codebooks):
    """[n, m, 256] float64: r_j . cb_jc - 1/2 ||cb_jc||^2 (its argmax over c is the nearest codeword in L2)."""
    m, _, dsub = codebooks.shape
    r = np.asarray(resid, dtype=np.float64).reshape(resid.shape[0], m, dsub)
    cb = np.asarray(codebooks, dtype=np.float64)
    return np.einsum("njt,jct->njc", r, cb) - 0.5 * (cb * cb).sum(axis=2)[None]


def encode(resid, codebooks):
    """[n, m] uint8, ties to the lowest codeword."""
    return sub_scores(resid, codebooks).argmax(axis=2).astype(np.uint8)


def lloyd_update(resid, codes, codebooks):
    """One Lloyd update in float64: the mean of the sub-vectors assigned to each (j, c); an empty codeword keeps its value.
    -> (codebooks [m,256,dsub] float64, counts [m,256])."""
    m, _, dsub = codebooks.shape
    r = np.asarray(resid, dtype=np.float64).reshape(resid.shape[0], m, dsub)
    out = np.asarray(codebooks, dtype=np.float64).copy()
    counts = np.zeros((m, KSUB), dtype=np.int64)
    for j in range(m):
        counts[j] = np.bincount(codes[:, j], minlength=KSUB)
        sums = np.zeros((KSUB, dsub))
        np.add.at(sums, codes[:, j], r[:, j])
        full = counts[j] > 0
        out[j, full] = sums[full] / counts[j, full, None]
    return out, counts


def initial_codebooks(resid, m):
    """[m,256,dsub]: codeword c of every sub-space is the sub-vector of training row c."""
    n, d = resid.shape
    return np.ascontiguousarray(np.asarray(resid[:KSUB]).reshape(KSUB, m, d // m).transpose(1, 0, 2))


def training_rows(n, seed):
    """The rows the codebooks are trained on, in order: the first 65,536 of a seeded host permutation."""
    return np.random.default_rng(seed).permutation(n)[:MAX_TRAIN_ROWS]


def train(resid, m, niter=10, init=None):
    """The trainer's iteration in float64 on the training residuals (already selected by training_rows): from `init`
    (default initial_codebooks), niter times encode + lloyd_update."""
    cb = np.asarray(initial_codebooks(resid, m) if init is None else init, dtype=np.float64)
    for _ in range(niter):
        cb, _ = lloyd_update(resid, encode(resid, cb), cb)
    return cb


def distortion(resid, codebooks):
    """Mean squared reconstruction error of the residuals under their nearest codewords (float64)."""
    m, _, dsub = codebooks.shape
    r = np.asarray(resid, dtype=np.float64).reshape(resid.shape[0], m, dsub)
    s = sub_scores(resid, codebooks).max(axis=2)                   # ||r - cb||^2 = ||r||^2 - 2 s
    return float(((r * r).sum(axis=2) - 2.0 * s).sum(axis=1).mean())


def lut(Q, codebooks):
    """[nq, m, 256] float64: q_j . cb_jc."""
    m, _, dsub = codebooks.shape
    q = np.asarray(Q, dtype=np.float64).reshape(Q.shape[0], m, dsub)
    return np.einsum("qjt,jct->qjc", q, np.asarray(codebooks, dtype=np.float64))


def decode(codes, list_of_row, centroids, codebooks, dtype=np.float32):
    """c_l + concat_j cb[j][code_j], computed in `dtype`."""
    m = codebooks.shape[0]
    cw = np.concatenate([np.asarray(codebooks, dtype=dtype)[j, codes[:, j]] for j in range(m)], axis=1)
    return (np.asarray(centroids, dtype=dtype)[list_of_row] + cw).astype(dtype)


def list_of_rows(list_off):
    return np.repeat(np.arange(len(list_off) - 1), np.diff(list_off))


def scan(codes, list_off, ids, lut_f32, probes, bias_f32, k):
    """The list scan: (D [nq,k] float32, I [nq,k] int64).  Scores accumulate in float32 in the contract's order; probes < 0
    are skipped; results by (-score, position), (-3.4028235e38, -1) padding."""
    lut_f32 = np.asarray(lut_f32, dtype=np.float32)
    bias_f32 = np.asarray(bias_f32, dtype=np.float32)
    nq, m, _ = lut_f32.shape
    D = np.full((nq, k), NEG, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        pos, acc = [], []
        for p, l in enumerate(probes[q]):
            if l < 0 or list_off[l + 1] == list_off[l]:
                continue
            rows = np.arange(list_off[l], list_off[l + 1])
            a = np.full(rows.shape, bias_f32[q, p], dtype=np.float32)
            for j in range(m):
                a = a + lut_f32[q, j][codes[rows, j]]              # float32 + float32, one j at a time
            assert a.dtype == np.float32
            pos.append(rows)
            acc.append(a)
        if not pos:
            continue
        pos, acc = np.concatenate(pos), np.concatenate(acc)
        order = np.lexsort((pos, -acc.astype(np.float64)))[:k]
        D[q, :len(order)] = acc[order]
        I[q, :len(order)] = pos[order] if ids is None else ids[pos[order]]
    return D, I


def spherical_kmeans(x, nlist, seed, niter=10):
    """A plain coarse quantizer for CPU-side studies (tests/golden/ivfpq_quality.json): seeded initial rows, assignment by
    inner product, unit-norm means, an empty cell keeps its centroid.  Not the GPU trainer's bits — only the same method."""
    x = np.asarray(x, dtype=np.float32)
    c = x[np.random.default_rng(seed).permutation(x.shape[0])[:nlist]].copy()
    for _ in range(niter):
        a = (x @ c.T).argmax(axis=1)
        sums = np.zeros((nlist, x.shape[1]))
        np.add.at(sums, a, x)
        full = np.bincount(a, minlength=nlist) > 0
        c[full] = (sums[full] / np.linalg.norm(sums[full], axis=1, keepdims=True)).astype(np.float32)
    return c


def clustered_unit_rows(n, d, centres, noise, seed, return_centres=False):
    """n seeded unit rows around `centres` unit centres, noise / sqrt(d) per coordinate, re-normalised."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = c[rng.integers(0, centres, n)] + (noise / np.sqrt(d)) * rng.standard_normal((n, d))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return (x, c.astype(np.float32)) if return_centres else x

"""numpy restatement of IndexPQ<m> and its R8 / R16 forms (wise_amd/index/flat_pq.py, include/wise_hip.h: wise_pqflat_*) the tests
hold the kernels and the classes to.  A test helper beside tests/ivfpq_ref.py: imported by tests only, never by wise_amd/.

An exhaustive product-quantizer index is one inverted list without a centroid, so everything here is the inverted-file restatement
asked the degenerate question:

  scores, scan        ivfpq_ref.scan over ONE list that holds every row, bias +0: acc = +0, then acc = acc + lut[j][code_j] for
                      j = 0 .. m-1 in float32 — the contract of wise_pqflat_topk; by (-score, position), (-3.4028235e38, -1) padding
  scan_pos            the same over chosen positions, through sel_ref.filtered_topk
  decode              concat_j cb[j][code_j], exact copies; NaN rows for positions outside [0, N)
  search_refine       ivfpq_refine_ref.refine of scan's positions: what IndexPQ<m>R8 / R16 return
  lut_f32             the table as wise_pq_lut computes it: one fmaf chain per entry from +0, in float32
  encode_f32, update_f32, train_f32
                      the trainer in the arithmetic of wise_pq_encode / wise_pq_update (csrc/ivf_pq.hip), float32: an fmaf chain per
                      (row, codeword) minus half the codeword's squared norm (itself 0.5 x an fmaf chain), the first best codeword
                      wins; a codeword's new value is the float32 sum of its rows IN ROW ORDER divided by their number.  fmaf(a, b, c)
                      is computed as float32(float64(a) float64(b) + float64(c)): the product is exact in float64, so the one
                      difference from a true fused operation is a double rounding, which needs the 53-bit sum to land exactly on a
                      float32 midpoint (about one operation in 2^29)
  recall_study        the quality study of tests/golden/pq_flat_quality.json (CPU only): `python tests/pq_flat_ref.py` rewrites it
"""
import numpy as np

import ivfpq_ref
import ivfpq_refine_ref
import sel_ref

KSUB = 256
NEG = np.float32(-3.4028234663852886e38)


# ---- the scan ---------------------------------------------------------------------------------------------------------------
def scores(codes, lut_f32):
    """[nq, N] float32 in the contract's order."""
    lut_f32 = np.asarray(lut_f32, dtype=np.float32)
    nq, m, _ = lut_f32.shape
    out = np.zeros((nq, codes.shape[0]), dtype=np.float32)
    for q in range(nq):
        a = np.zeros(codes.shape[0], dtype=np.float32)                 # +0.0f
        for j in range(m):
            a = a + lut_f32[q, j][codes[:, j]]                         # float32 + float32, one j at a time
        assert a.dtype == np.float32
        out[q] = a
    return out


def scan(codes, ids, lut_f32, k, id_base=0):
    """(D [nq,k] float32, I [nq,k] int64) of wise_pqflat_topk: ivfpq_ref.scan over one list of all rows, one probe, bias +0.
    ids None: id_base + position."""
    N, nq = codes.shape[0], np.asarray(lut_f32).shape[0]
    list_off = np.array([0, N], dtype=np.int64)
    D, P = ivfpq_ref.scan(codes, list_off, None, lut_f32, np.zeros((nq, 1), dtype=np.int64), np.zeros((nq, 1), dtype=np.float32), k)
    if ids is None or N == 0:
        return D, np.where(P >= 0, P + id_base, -1)
    return D, np.where(P >= 0, np.asarray(ids, dtype=np.int64)[np.maximum(P, 0)], -1)


def scan_pos(codes, ids, lut_f32, pos, k, id_base=0):
    """(D, I) of wise_pqflat_topk_pos over the ascending positions pos: sel_ref.filtered_topk of their scores."""
    pos = np.asarray(pos, dtype=np.int64)
    D, I, _ = sel_ref.filtered_topk(scores(codes[pos], lut_f32), pos, np.ones(codes.shape[0], dtype=bool), ids, k)
    return D, (np.where(I >= 0, I + id_base, -1) if ids is None else I)


def decode(codes, pos, codebooks):
    """[len(pos), d] float32: the codewords of row pos[i] side by side; NaN where pos[i] is outside [0, N)."""
    m, _, dsub = codebooks.shape
    pos = np.asarray(pos, dtype=np.int64)
    ok = (pos >= 0) & (pos < codes.shape[0])
    out = np.full((len(pos), m * dsub), np.nan, dtype=np.float32)
    c = codes[pos[ok]]
    out[ok] = np.concatenate([np.asarray(codebooks, dtype=np.float32)[j, c[:, j]] for j in range(m)], axis=1)
    return out


def search_refine(codes, ids, lut_f32, rows, kind, scales, Q, k, k_factor, pos=None):
    """(D, I) of an IndexPQ<m>R8 / R16 search: the max(k, min(k k_factor, 2048)) best positions of the PQ scan (over pos where given),
    re-scored by ivfpq_refine_ref.refine."""
    kc = max(k, min(k * max(k_factor, 1), 2048))
    _, cand = scan(codes, None, lut_f32, kc) if pos is None else scan_pos(codes, None, lut_f32, pos, kc)
    return ivfpq_refine_ref.refine(rows, kind, scales, ids, Q, cand, k)


# ---- float32 arithmetic of the trainer's kernels ---------------------------------------------------------------------------------
def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def lut_f32(Q, codebooks):
    """[nq, m, 256] float32: lut[q, j, c] = the fmaf chain over i of q[j dsub + i] cb[j, c, i] from +0 (wise_pq_lut)."""
    cb = np.asarray(codebooks, dtype=np.float32)
    m, _, dsub = cb.shape
    q = np.asarray(Q, dtype=np.float32).reshape(-1, m, dsub)
    a = np.zeros((q.shape[0], m, KSUB), dtype=np.float32)
    for i in range(dsub):
        a = _fma(q[:, :, None, i], cb[None, :, :, i], a)
    return a


def encode_f32(rows, codebooks, chunk=4096):
    """[n, m] uint8 as wise_pq_encode gives them."""
    cb = np.asarray(codebooks, dtype=np.float32)
    m, _, dsub = cb.shape
    half = np.zeros((m, KSUB), dtype=np.float32)
    for i in range(dsub):
        half = _fma(cb[:, :, i], cb[:, :, i], half)
    half = np.float32(0.5) * half
    rows = np.asarray(rows, dtype=np.float32)
    out = np.empty((rows.shape[0], m), dtype=np.uint8)
    for s in range(0, rows.shape[0], chunk):
        r = rows[s:s + chunk].reshape(-1, m, dsub)
        a = np.zeros((r.shape[0], m, KSUB), dtype=np.float32)
        for i in range(dsub):
            a = _fma(r[:, :, None, i], cb[None, :, :, i], a)
        a = a - half[None]
        assert a.dtype == np.float32
        out[s:s + chunk] = a.argmax(axis=2)                            # the first of equal bests: `>` in ascending c
    return out


def update_f32(rows, codes, codebooks):
    """[m, 256, dsub] float32 as wise_pq_update gives them: per codeword the float32 sum of its rows in ascending row order over
    their count; an empty codeword keeps its value."""
    cb = np.asarray(codebooks, dtype=np.float32)
    m, _, dsub = cb.shape
    r = np.asarray(rows, dtype=np.float32).reshape(-1, m, dsub)
    out = cb.copy()
    for j in range(m):
        c = codes[:, j].astype(np.int64)
        order = np.argsort(c, kind="stable")                          # by codeword, row order within one
        cs = c[order]
        counts = np.bincount(cs, minlength=KSUB)
        first = np.concatenate([[0], np.cumsum(counts)[:-1]])
        rank = np.arange(len(cs)) - first[cs]                          # a row's number among its codeword's rows
        acc = np.zeros((KSUB, dsub), dtype=np.float32)
        for t in range(int(counts.max()) if len(cs) else 0):
            sel = order[rank == t]                                     # at most one row per codeword
            acc[c[sel]] = acc[c[sel]] + r[sel, j]
        full = counts > 0
        out[j, full] = acc[full] / counts[full, None].astype(np.float32)
    assert out.dtype == np.float32
    return out


def train_f32(rows, m, niter=10):
    """The trainer on the training rows (already selected and ordered by ivfpq_ref.training_rows): the first 256 rows are the
    initial codewords, then niter times encode_f32 + update_f32."""
    rows = np.asarray(rows, dtype=np.float32)
    cb = ivfpq_ref.initial_codebooks(rows, m).astype(np.float32)
    for _ in range(niter):
        cb = update_f32(rows, encode_f32(rows, cb), cb)
    return cb


# ---- the recall study of tests/golden/pq_flat_quality.json (CPU only) -----------------------------------------------------------
STUDY = dict(rows=60000, dim=128, m=16, centres=122, noise=0.35, k=10, queries=64, niter=10, k_factors=(5, 10, 20, 50, 100))


def recall_study(seed, cfg=STUDY):
    """recall@k against the float64 flat answer on the clustered study set of ivfpq_refine_ref (the same rows and queries per seed):
    of the PQ scan alone and after re-ranking its k * k_factor best positions by each store.  The codebooks are trained on the rows
    themselves (rows perm[:65536] of the seeded permutation, float64 restatement).  -> dict of floats / per-k_factor dicts."""
    N, d, m, k, nq = cfg["rows"], cfg["dim"], cfg["m"], cfg["k"], cfg["queries"]
    X, _ = ivfpq_refine_ref.clustered_rows_like_the_bench(N, d, cfg["centres"], cfg["noise"], seed)
    rng = np.random.default_rng(seed + 1000)
    e = rng.standard_normal((nq, d))
    Q = X[:nq] + 0.05 * e / np.linalg.norm(e, axis=1, keepdims=True)
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    tr = X[ivfpq_ref.training_rows(N, 1234)]
    cb = ivfpq_ref.initial_codebooks(tr, m).astype(np.float64)
    for _ in range(cfg["niter"]):                              # ivfpq_ref.train with the assignment step taken a chunk at a time
        cb, _ = ivfpq_ref.lloyd_update(tr, np.concatenate([ivfpq_ref.encode(tr[s:s + 8192], cb) for s in range(0, N, 8192)]), cb)
    cb = cb.astype(np.float32)
    codes = np.concatenate([ivfpq_ref.encode(X[s:s + 8192], cb) for s in range(0, N, 8192)])
    kc = k * max(cfg["k_factors"])
    _, cand = scan(codes, None, ivfpq_ref.lut(Q, cb).astype(np.float32), kc)
    exact = X.astype(np.float64) @ Q.astype(np.float64).T      # [N, nq]
    If = np.stack([np.lexsort((np.arange(N), -exact[:, q]))[:k] for q in range(nq)])
    out = {"pq_alone": ivfpq_refine_ref._recall(cand[:, :k], If)}
    for kind in (8, 16):
        rows, scales = ivfpq_refine_ref.quantise(X, kind)
        out[f"r{kind}"] = {str(f): ivfpq_refine_ref._recall(ivfpq_refine_ref.refine(rows, kind, scales, None, Q, cand[:, :k * f], k)[1], If)
                           for f in cfg["k_factors"]}
    return out


study_summary = ivfpq_refine_ref.study_summary     # the smallest gain over PQ alone at k_factor 50 and its spread, per store


if __name__ == "__main__":      # python tests/pq_flat_ref.py: recompute tests/golden/pq_flat_quality.json
    import json
    from pathlib import Path

    seeds = [0, 1, 2, 3, 4]
    runs = []
    for s in seeds:
        runs.append(recall_study(s))
        print(s, json.dumps(runs[-1]), flush=True)
    gold = {"what": "pq_flat_ref.recall_study (numpy restatements only, no GPU) for five seeds: " + json.dumps(STUDY)
                    + "; recall@10 against the float64 flat answer; gains are taken at k_factor 50",
            "seeds": seeds, "runs": runs, **study_summary(runs)}
    (Path(__file__).resolve().parent / "golden" / "pq_flat_quality.json").write_text(json.dumps(gold, indent=1) + "\n")

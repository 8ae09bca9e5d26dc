"""numpy restatement of IndexIVFFlatL2 (include/wise_hip.h: wise_ivfl2_*, wise_ivf_l2_coarse, wise_ivf_list_means) the tests hold the
kernels and the index to.  A test helper beside tests/l2_flat_ref.py: imported by tests only, never by wise_amd/.

THE DISTANCE is l2_flat_ref.dists: a row of a list scores what IndexFlatL2 gives the same (query, row).
THE COARSE RULE: g(x, c) = fl(s(x, c) - h_c); s = +0, then s = fma32(x[i], c[i], s) for i = 0 .. d - 1 in order (wise_ip_scores_f32);
h_c = l2_flat_ref.half_norms(c).  A row goes to argmax_c g (ties: the lowest c); a query probes the nprobe largest g (ties: the lower
c), written in ascending list order, -1 padding when nprobe > nlist.
THE SCAN: the k smallest distances over the rows of the probed lists (probes < 0 or >= nlist and empty lists skipped), ties by the
lower position, padding (+3.4028235e38, -1).  Range: every such row with dist < radius, strictly.
THE TRAINER: seeds = the rows at torch.randperm(n, seed 1234)[:nlist] as they are; an iteration = assignment by the coarse rule, the
rows grouped by list in row order, per list the float32 sum of its rows in that order, sum / (float)count (an empty cell keeps its
zeros), then every empty cell becomes its donor's mean * (1 + 1e-3 sign(.)), donors = the fullest cells (ties: the lower cell first).
"""
import numpy as np

import l2_flat_ref
from ivfsq_ref import fma32

PAD = l2_flat_ref.PAD


def ip_chain(X, C):
    """[n, nlist] float32: s(x, c), the index-ordered fmaf chain from +0"""
    X, C = np.asarray(X, dtype=np.float32), np.asarray(C, dtype=np.float32)
    s = np.zeros((X.shape[0], C.shape[0]), dtype=np.float32)
    for i in range(X.shape[1]):
        s = fma32(X[:, i][:, None], C[:, i][None, :], s).reshape(s.shape)
    return s


def coarse_scores(X, C):
    """[n, nlist] float32: g(x, c) = fl(s(x, c) - h_c)"""
    g = ip_chain(X, C) - l2_flat_ref.half_norms(C)[None, :]
    assert g.dtype == np.float32
    return g


def assign(X, C, G=None):
    """[n] int64: argmax_c g, ties to the lowest c"""
    G = coarse_scores(X, C) if G is None else G
    return np.argmax(G, axis=1).astype(np.int64)


def probes(Q, C, nprobe, G=None):
    """[nq, nprobe] int64: the nprobe largest g per query (ties: the lower list), in ascending list order, -1 padding"""
    G = coarse_scores(Q, C) if G is None else G
    nq, nlist = G.shape
    out = np.full((nq, nprobe), -1, dtype=np.int64)
    for q in range(nq):
        best = np.sort(np.lexsort((np.arange(nlist), -G[q].astype(np.float64)))[:nprobe])
        out[q, :len(best)] = best
    return out


def candidates(list_off, probes_q, keep=None):
    """positions of the rows of one query's probed lists, in probe order, then ascending (a list named twice is listed twice)"""
    nlist = len(list_off) - 1
    pos = [np.zeros(0, dtype=np.int64)]
    for l in probes_q:
        if 0 <= l < nlist and list_off[l + 1] > list_off[l]:
            pos.append(np.arange(list_off[l], list_off[l + 1], dtype=np.int64))
    pos = np.concatenate(pos)
    return pos if keep is None else pos[np.asarray(keep, dtype=bool)[pos]]


def scan(X, list_off, ids, Q, probes, k, keep=None, S=None, pos_base=0):
    """(D [nq,k] float32 ascending, I [nq,k] int64) of wise_ivfl2_scan (keep: bool [N]: wise_ivfl2_scan_sel); ids None -> pos_base +
    position.  S: l2_flat_ref.dists(X, Q) if already known."""
    S = l2_flat_ref.dists(X, Q) if S is None else S
    nq = probes.shape[0]
    D = np.full((nq, k), PAD, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        pos = candidates(list_off, probes[q], keep)                 # (a list named twice competes twice, as in the other scans)
        s = S[q, pos]
        order = np.lexsort((pos, s))[:k]
        D[q, :len(order)] = s[order]
        I[q, :len(order)] = pos[order] + pos_base if ids is None else ids[pos[order]]
    return D, I


def range_raw(X, list_off, Q, probes, radius, keep=None, S=None):
    """(lims, D, P) as wise_ivfl2_range_fill writes them with ids == NULL: per query the hits (dist < radius) in probe order, then
    ascending position."""
    S = l2_flat_ref.dists(X, Q) if S is None else S
    r = np.float32(radius)
    lims, Ds, Ps = [0], [], []
    for q in range(probes.shape[0]):
        pos = candidates(list_off, probes[q], keep)
        pos = pos[S[q, pos] < r]
        Ds.append(S[q, pos])
        Ps.append(pos)
        lims.append(lims[-1] + len(pos))
    return np.asarray(lims, dtype=np.int64), np.concatenate(Ds).astype(np.float32), np.concatenate(Ps).astype(np.int64)


def range_search(X, list_off, ids, Q, probes, radius, keep=None, S=None):
    """(lims, D, I) of IVFFlatL2Index.range_search: every segment by ascending distance, ties by ascending position"""
    S = l2_flat_ref.dists(X, Q) if S is None else S
    lims, D, P = range_raw(X, list_off, Q, probes, radius, keep, S)
    for q in range(len(lims) - 1):
        a, b = lims[q], lims[q + 1]
        order = np.lexsort((P[a:b], D[a:b]))
        D[a:b], P[a:b] = D[a:b][order], P[a:b][order]
    return lims, D, (P if ids is None else np.asarray(ids)[P])


def list_sums(X, a, nlist):
    """[nlist, d] float32: per list the sum of its rows in row order, one float32 addition per row and element"""
    X = np.asarray(X, dtype=np.float32)
    sums = np.zeros((nlist, X.shape[1]), dtype=np.float32)
    for r in np.argsort(a, kind="stable"):
        sums[a[r]] = sums[a[r]] + X[r]
    return sums


def list_means(sums, counts):
    """sums / (float32)counts, one float32 division per element; rows with count 0 as they are"""
    out = np.array(sums, dtype=np.float32)
    full = np.asarray(counts) > 0
    out[full] = out[full] / np.asarray(counts)[full].astype(np.float32)[:, None]
    assert out.dtype == np.float32
    return out


def reseed(cells, counts):
    """every empty cell = its donor's row * (1 + 1e-3 sign(.)); donors: the fullest cells, ties the lower cell first"""
    counts = np.asarray(counts)
    empty = np.flatnonzero(counts == 0)
    donors = np.argsort(-counts, kind="stable")[:empty.size]
    out = cells.copy()
    for e, s in zip(empty, donors):
        v = cells[s]
        out[e] = v * (np.float32(1.0) + np.float32(1e-3) * np.sign(v).astype(np.float32))
    assert out.dtype == np.float32
    return out


def train_iteration(X, C):
    """one iteration of the plain k-means: the next centroids [nlist, d] float32"""
    a = assign(X, C)
    counts = np.bincount(a, minlength=C.shape[0])
    return reseed(list_means(list_sums(X, a, C.shape[0]), counts), counts)


def seeds(X, nlist, seed=1234):
    import torch

    perm = torch.randperm(X.shape[0], generator=torch.Generator(device="cpu").manual_seed(seed))[:nlist].numpy()
    return np.asarray(X, dtype=np.float32)[perm].copy()


def train(X, nlist, niter=10, seed=1234):
    C = seeds(X, nlist, seed)
    for _ in range(niter):
        C = train_iteration(X, C)
    return C


def build(X, C):
    """(order, list_off): the rows grouped by list, stable — position p of the index holds row order[p]"""
    a = assign(X, C)
    order = np.argsort(a, kind="stable")
    list_off = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=C.shape[0]))]).astype(np.int64)
    return order, list_off


def long_rows(n, d, seed, spread=4.0, centres=0, noise=0.3):
    """[n, d] float32 rows that are NOT normalised: directions (around `centres` clusters when given) times lengths log-uniform
    over [1, spread]"""
    rng = np.random.default_rng(seed)
    if centres:
        c = rng.standard_normal((centres, d))
        c /= np.linalg.norm(c, axis=1, keepdims=True)
        e = rng.standard_normal((n, d))
        u = c[rng.integers(0, centres, size=n)] + noise * e / np.linalg.norm(e, axis=1, keepdims=True)
    else:
        u = rng.standard_normal((n, d))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (u * np.exp(rng.uniform(0.0, np.log(spread), size=(n, 1)))).astype(np.float32)


# ---- the recall study of tests/golden/ivf_l2_quality.json (CPU only; tools/make_golden_ivf_l2_quality.py) ------------------------
# 60,000 x 128 rows around nlist / 2 centres (the set of ivfsq_ref.recall_study) times lengths log-uniform over [1, 4]; queries beside
# rows; nprobe 32.  The METHOD of the index, not its bits: scores are numpy's float32 products, as in the sibling studies.
STUDY = dict(rows=60000, dim=128, nlist=244, noise=0.35, nprobe=32, k=10, queries=64, spread=4.0, niter=10, more_nprobes=(1, 4))


def _recall(I, If):
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / len(b) for a, b in zip(I, If)]))


def plain_kmeans(x, nlist, seed, niter=10):
    """The trainer's method on the host: seeded rows as they are, assignment to the largest x . c - |c|^2 / 2, means; an empty cell
    keeps its centroid (the GPU trainer re-seeds it: none is empty in the study)."""
    x = np.asarray(x, dtype=np.float32)
    c = x[np.random.default_rng(seed).permutation(x.shape[0])[:nlist]].copy()
    for _ in range(niter):
        a = (x @ c.T - 0.5 * (c * c).sum(axis=1)[None, :]).argmax(axis=1)
        sums = np.zeros((nlist, x.shape[1]))
        np.add.at(sums, a, x)
        cnt = np.bincount(a, minlength=nlist)
        full = cnt > 0
        c[full] = (sums[full] / cnt[full][:, None]).astype(np.float32)
    return c


def _probed_recall(X64, Q64, exact, a, coarse, nprobe, k, If):
    """recall@k of the exact L2 answer within the rows of the nprobe lists of largest `coarse` [nq, nlist] (a: the rows' lists)"""
    probes = np.argsort(-coarse, axis=1, kind="stable")[:, :nprobe]
    I, share = [], []
    for q in range(Q64.shape[0]):
        rows = np.flatnonzero(np.isin(a, probes[q]))
        I.append(rows[np.lexsort((rows, exact[q, rows]))[:k]])
        share.append(len(rows) / len(a))
    return _recall(I, If), float(np.mean(share))


def recall_study(seed, cfg=STUDY):
    """recall@k against the float64 exact L2 answer on one seeded set of rows that are not normalised: of IndexIVFFlatL2 (plain
    k-means, the L2 coarse rule) and, beside it, of the spherical inner-product coarse quantizer of the other inverted-file types
    over the same rows (unit centroids, assignment and probes by the largest inner product, exact L2 distances within the probed
    lists); the share of the rows each scans.  -> dict of floats."""
    import ivfpq_ref
    from ivfpq_refine_ref import clustered_rows_like_the_bench

    N, d, nlist, k, nq, nprobe = cfg["rows"], cfg["dim"], cfg["nlist"], cfg["k"], cfg["queries"], cfg["nprobe"]
    U, _ = clustered_rows_like_the_bench(N, d, max(nlist // 2, 16), cfg["noise"], seed)
    rng = np.random.default_rng(seed + 1000)
    X = (U * np.exp(rng.uniform(0.0, np.log(cfg["spread"]), size=(N, 1)))).astype(np.float32)
    e = rng.standard_normal((nq, d))
    Q = (X[:nq] + 0.05 * np.linalg.norm(X[:nq], axis=1, keepdims=True) * e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32)
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    exact = (Q64 * Q64).sum(axis=1)[:, None] + (X64 * X64).sum(axis=1)[None, :] - 2.0 * (Q64 @ X64.T)
    If = np.stack([np.lexsort((np.arange(N), exact[q]))[:k] for q in range(nq)])
    c2 = plain_kmeans(X, nlist, 1234, cfg["niter"])
    h2 = 0.5 * (c2.astype(np.float64) ** 2).sum(axis=1)
    a2 = (X64 @ c2.astype(np.float64).T - h2[None, :]).argmax(axis=1)
    g2 = Q64 @ c2.astype(np.float64).T - h2[None, :]
    r2, s2 = _probed_recall(X64, Q64, exact, a2, g2, nprobe, k, If)
    cs = ivfpq_ref.spherical_kmeans(X, nlist, 1234, cfg["niter"])
    as_ = (X64 @ cs.astype(np.float64).T).argmax(axis=1)
    gs = Q64 @ cs.astype(np.float64).T
    rs, ss = _probed_recall(X64, Q64, exact, as_, gs, nprobe, k, If)
    ip = np.stack([np.lexsort((np.arange(N), -(X64 @ Q64[q])))[:k] for q in range(nq)])
    out = {"ivfflat_l2": r2, "spherical_ip_coarse": rs, "scanned_share_l2": s2, "scanned_share_spherical": ss,
           "empty_cells_l2": int((np.bincount(a2, minlength=nlist) == 0).sum()), "ip_top10_overlap_with_l2": _recall(ip, If)}
    for p in cfg["more_nprobes"]:                                  # beside the study's nprobe: where the two part, if they do
        out[f"ivfflat_l2_nprobe{p}"] = _probed_recall(X64, Q64, exact, a2, g2, p, k, If)[0]
        out[f"spherical_ip_coarse_nprobe{p}"] = _probed_recall(X64, Q64, exact, as_, gs, p, k, If)[0]
    return out

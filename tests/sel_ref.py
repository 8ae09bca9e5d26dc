"""numpy restatement of a search restricted to a set of ids (wise_amd/index/selector.py) that the tests hold the kernels to.
A test helper: imported by tests only, never by wise_amd/.

  resolve         a selector -> the boolean mask by row position
  bitmap          that mask as the uint32 words wise_sel_bitmap writes
  filtered_topk   the k best masked rows by (-score, position), the project's padding
  pq_scan         ivfpq_ref.scan restricted to the masked positions: the scan asked for every probed row (k = their number), the
                  unselected positions dropped, cut to k — the contract-order fp32 scores without restating them
"""
import numpy as np

import ivfpq_ref

NEG = np.float32(-3.4028234663852886e38)


def resolve(ids_of_rows, selector):
    """[N] bool: row p is selected iff its external id ids_of_rows[p] is.  The selector is read by its public attributes:
    `.ids` (batch), `.imin` / `.imax` (range), `.sel` (not)."""
    ids_of_rows = np.asarray(ids_of_rows, dtype=np.int64)
    if hasattr(selector, "sel"):
        return ~resolve(ids_of_rows, selector.sel)
    if hasattr(selector, "imin"):
        return (ids_of_rows >= selector.imin) & (ids_of_rows < selector.imax)
    return np.isin(ids_of_rows, np.asarray(selector.ids, dtype=np.int64))


def bitmap(mask):
    """uint32[ceil(N / 32)]: bit (p & 31) of word p >> 5 = mask[p]; the bits past N are zero."""
    mask = np.asarray(mask, dtype=bool)
    padded = np.zeros((mask.size + 31) // 32 * 32, dtype=bool)
    padded[:mask.size] = mask
    return np.packbits(padded.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)


def filtered_topk(scores, positions, mask, ids, k):
    """scores [nq, n] of the rows at `positions` [n] (ascending positions of the index) -> (D [nq,k] float32, I [nq,k] int64,
    P [nq,k] int64 positions): the k best rows with mask[position] set, by (-score, position); padding (-3.4028235e38, -1).
    ids: [N] external ids by position, or None for the positions themselves.  The order is decided on the scores as given
    (pass float64 scores for a float64 order); D holds them rounded to float32."""
    scores = np.asarray(scores)
    positions = np.asarray(positions, dtype=np.int64)
    nq = scores.shape[0]
    D = np.full((nq, k), NEG, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    P = np.full((nq, k), -1, dtype=np.int64)
    live = np.flatnonzero(np.asarray(mask, dtype=bool)[positions])
    for q in range(nq):
        s = scores[q, live].astype(np.float64)
        order = live[np.lexsort((positions[live], -s))[:k]]
        D[q, :order.size] = scores[q, order]
        P[q, :order.size] = positions[order]
        I[q, :order.size] = positions[order] if ids is None else np.asarray(ids)[positions[order]]
    return D, I, P


def pq_scan(codes, list_off, ids, lut_f32, probes, bias_f32, k, mask):
    """ivfpq_ref.scan among the rows with mask[position] set: (D [nq,k] float32 in the contract's bits, I [nq,k] int64)."""
    nq = probes.shape[0]
    sizes = np.diff(list_off)
    D = np.full((nq, k), NEG, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    mask = np.asarray(mask, dtype=bool)
    for q in range(nq):
        pr = probes[q:q + 1]
        rows = int(sizes[pr[pr >= 0]].sum())          # a list probed twice is scanned twice, as the kernel does
        if rows == 0:
            continue
        Dq, Pq = ivfpq_ref.scan(codes, list_off, None, lut_f32[q:q + 1], pr, bias_f32[q:q + 1], rows)
        keep = np.flatnonzero((Pq[0] >= 0) & mask[np.maximum(Pq[0], 0)])[:k]
        D[q, :keep.size] = Dq[0, keep]
        I[q, :keep.size] = Pq[0, keep] if ids is None else np.asarray(ids)[Pq[0, keep]]
    return D, I


# ---- the flat cases of tests/test_gpu_select.py: data, selectors and the near-tie rule, kept here so that the CPU suite can hold
# the seeds to the rule's 1 % cap without a GPU
FLAT_SEEDS = {}            # (N, d) -> seed of the queries (the rows' seed is N + d), chosen on the CPU for the 1 % cap; filled below
SELECTIVITIES = ("all", "tenth", "thousandth", "one", "none")
# Two oracle (float64) scores closer than this are a near-tie whose order the fp32 scan is not held to.  The rows and queries
# are unit vectors, so a score and every partial sum of it is below 1 in magnitude and one fp32 rounding moves it by at most
# 2^-24; 2^-22 is four such roundings, two for each score of a pair.  This is the number format's step, not a worst case: the
# worst-case bound of an fp32 dot product of d = 768 terms (18 roundings along the scan's path times sum |q_i x_i| ~ 0.64, 7e-7
# per score) would leave out ~3 % of the ranks at N = 300000, k = 100, where neighbouring oracle scores lie 1e-4 apart.
NEAR_TIE = 2.0 ** -22


def unit_rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def flat_case(N, d):
    """(X [N,d], Q [8,d], ids [N]) of the flat case (N, d): unit rows, unit queries, external ids that are not the positions."""
    X = unit_rows(N, d, N + d)
    Q = unit_rows(8, d, FLAT_SEEDS[(N, d)])
    ids = np.random.default_rng(N * 7 + d).permutation(N).astype(np.int64) * 3 + 11
    return X, Q, ids


def flat_selector_spec(ids, which):
    """What selects the rows of selectivity `which`, as (kind, arguments) — the tests build the selector objects from it:
    all = a range over every id; tenth = the complement of a batch of nine tenths of the ids; thousandth = a batch (with
    duplicates and ids no row carries); one = a batch of one id; none = a batch of ids no row carries."""
    N = ids.size
    rng = np.random.default_rng(N + 5)
    if which == "all":
        return "range", (int(ids.min()), int(ids.max()) + 1)
    if which == "tenth":
        return "not_batch", (rng.permutation(ids)[: N - N // 10],)
    if which == "thousandth":
        chosen = rng.permutation(ids)[: max(N // 1000, 1)]
        return "batch", (np.concatenate([chosen, chosen[:3], [-7, 1, 4]]),)           # ids are 2 mod 3: 1 and 4 are absent
    if which == "one":
        return "batch", ([int(ids[N // 2])],)
    return "batch", ([-7, 1, 4],)


def scores_f64(X, Q, chunk=65536):
    """[nq, N] float64 inner products (rows converted a chunk at a time)"""
    out = np.empty((Q.shape[0], X.shape[0]))
    Q64 = Q.astype(np.float64)
    for s in range(0, X.shape[0], chunk):
        out[:, s:s + chunk] = Q64 @ X[s:s + chunk].astype(np.float64).T
    return out


def near_tie_ranks(S64, mask, k):
    """[nq, k] bool: rank j of query q sits within NEAR_TIE of a neighbour in the oracle's order of the masked rows (the first
    row left out, rank k, counts as the last rank's neighbour).  Padding ranks are False."""
    nq = S64.shape[0]
    live = np.flatnonzero(mask)
    out = np.zeros((nq, k), dtype=bool)
    for q in range(nq):
        s = -np.sort(-S64[q, live])[:k + 1]
        close = np.diff(s) > -NEAR_TIE                      # close[j]: ranks j and j + 1
        n = min(k, s.size)
        out[q, :n] = np.concatenate([[False], close])[:n] | np.concatenate([close, [False]])[:n]
    return out


FLAT_SEEDS.update({(1000, 64): 7, (1000, 512): 7, (1000, 768): 7, (4096, 64): 7, (4096, 512): 7, (4096, 768): 8,
                   (300000, 64): 7, (300000, 512): 7, (300000, 768): 7})

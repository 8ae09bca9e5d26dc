"""-m gpu: search_grouped (csrc/group_topk.hip, the *_group_scores kernels, wise_amd/index/group_search.py) bit for bit.

(1) wise_group_best / wise_group_topk alone on synthetic ord arrays against tests/group_ref.py; (2) every supported index type end
    to end against an oracle the code under test does not touch: index.search(x, N) lists every candidate row in (score, position)
    order with the exact bits, and the first occurrence of each group in that list, cut to k, is the answer — also under selectors
    that leave groups without a row; (3) a grid of many blocks against group_ref fed with the scores of the types' restatements;
    (4) ties at block and segment boundaries; (5) argument errors leave the outputs untouched; (6) stale tables raise."""
import numpy as np
import pytest
import torch

import group_ref as gr
from wise_amd import _lib
from wise_amd.index.selector import IDSelectorBatch, IDSelectorRange, SearchParameters, SearchParametersIVF

pytestmark = pytest.mark.gpu
WISE_E_INVALID = -1


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same3(got, want):
    return all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))


def uneven_runs(rng, N, G, longest=400):
    """[N] int64: the group of every row — G contiguous runs of uneven length, from 1 row to `longest` where the sizes allow it"""
    length = np.ones(G, dtype=np.int64)
    extra = N - G
    if G > 2 and extra >= longest - 1:
        length[G // 3] = longest
        extra -= longest - 1
    if extra:
        others = np.flatnonzero(length == 1)[1:] if G > 1 else np.arange(1)       # one run keeps a single row
        length[others] += rng.multinomial(extra, rng.dirichlet(np.full(others.size, 0.3)))
    assert length.sum() == N and length.min() >= 1
    return np.repeat(np.arange(G, dtype=np.int64), length)


def tables_of(gid, G):
    """(gid int32, group_off, group_rows uint32) of a group assignment, as build_group_tables lays them out"""
    rows = np.argsort(gid, kind="stable")
    off = np.zeros(G + 1, dtype=np.int64)
    np.cumsum(np.bincount(gid, minlength=G), out=off[1:])
    return gid.astype(np.int32), off, rows.astype(np.uint32)


# ---- (1) stages 2 and 3 alone
@pytest.mark.parametrize("layout", ["runs", "random"])
@pytest.mark.parametrize("G", [1, 7, 700, 5000])
def test_group_best_and_topk_alone(G, layout):
    lib = _lib.lib()
    N = 5000
    rng = np.random.default_rng(G * 2 + (layout == "random"))
    gid = uneven_runs(rng, N, G)
    if layout == "random":
        gid = rng.permutation(gid)
    gid32, off, rows = tables_of(gid, G)
    group_keys = np.arange(G, dtype=np.int64) * 3 + 11
    ids = rng.permutation(N).astype(np.int64) + 1000
    st = _lib.stream_ptr()
    for nq in (1, 5):
        # few distinct values: equal images across and inside groups; zeros: absent rows; whole groups absent
        ord_ = (rng.integers(0, 6, size=(nq, N)) * 0x01000000 + 0x80000000).astype(np.uint32)
        ord_[rng.random((nq, N)) < 0.3] = 0
        for g in range(0, G, 5):
            ord_[nq - 1, gid == g] = 0
        want_best = gr.best_keys(ord_, gid, G)
        d_ord, d_off, d_rows = _dev(ord_.view(np.int32)), _dev(off), _dev(rows.view(np.int32))
        best = torch.full((nq, G), -1, dtype=torch.int64, device="cuda")
        _lib.check(lib.wise_group_best(d_ord.data_ptr(), N, nq, d_off.data_ptr(), d_rows.data_ptr(), G, best.data_ptr(), st), "wise_group_best")
        assert np.array_equal(best.cpu().numpy().view(np.uint64), want_best)
        d_gid, d_keys, d_ids = _dev(gid32), _dev(group_keys), _dev(ids)
        for k in (1, 10, 100, 2048):                                                # k > G: padding
            need = lib.wise_group_workspace_bytes(N, G, nq, k)
            assert need > 0
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            for flip, metric, use_ids in ((0, "ip", True), (1, "l2", False)):
                D = torch.empty(nq, k, dtype=torch.float32, device="cuda")
                I = torch.empty(nq, k, dtype=torch.int64, device="cuda")
                Gk = torch.empty(nq, k, dtype=torch.int64, device="cuda")
                _lib.check(lib.wise_group_topk(best.data_ptr(), G, nq, k, d_gid.data_ptr(), N, d_keys.data_ptr(),
                                               d_ids.data_ptr() if use_ids else 0, 0 if use_ids else 77, flip, D.data_ptr(), I.data_ptr(),
                                               Gk.data_ptr(), ws.data_ptr(), ws.numel(), st), "wise_group_topk")
                want = gr.select(want_best, k, gid, group_keys, ids if use_ids else None, 77, metric)
                assert _same3((D, I, Gk), want), (nq, k, flip)


# ---- (2) every supported type end to end
def _rows(N, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, d)).astype(np.float32)
    X[N // 2] = X[5]                                                                # equal scores in different groups and inside one
    X[6] = X[5]
    return X, rng


def _make_flat(name, d, X, ids):
    from wise_amd.index.flat_ip import FlatIPIndex
    from wise_amd.index.flat_l2 import FlatL2Index
    from wise_amd.index.flat_sq import FlatSQ8IPIndex, FlatSQfp16IPIndex, FlatSQfp16L2Index
    ix = {"IndexFlatIP": FlatIPIndex, "IndexSQfp16": FlatSQfp16IPIndex, "IndexSQ8bit": FlatSQ8IPIndex, "IndexFlatL2": FlatL2Index,
          "IndexSQfp16L2": FlatSQfp16L2Index}[name](d)
    if name == "IndexSQ8bit":
        ix.train(X)
    ix.add_with_ids(X, ids)
    return ix


def _make_ivf(name, d, nlist, X, ids):
    from wise_amd.index.ivf_flat import IVFFlatIPIndex, IVFFlatL2Index
    from wise_amd.index.ivf_sq import IVFSQfp16IPIndex, IVFSQIPIndex
    ix = {"IndexIVFFlat": IVFFlatIPIndex, "IndexIVFSQ8": IVFSQIPIndex, "IndexIVFSQfp16": IVFSQfp16IPIndex,
          "IndexIVFFlatL2": IVFFlatL2Index}[name](d, nlist)
    ix.train(X)
    ix.add_with_ids(X, ids)
    return ix


def _oracle(ix, x, k, key_of_id, params):
    """The first occurrence of each group in index.search(x, N), cut to k"""
    N = ix.ntotal
    D, I = ix.search(x, N, params=params)
    pad = np.float32(3.4028234663852886e38 if ix.metric == "l2" else -3.4028234663852886e38)
    oD = np.full((x.shape[0], k), pad, dtype=np.float32)
    oI = np.full((x.shape[0], k), -1, dtype=np.int64)
    oG = np.full((x.shape[0], k), -1, dtype=np.int64)
    for q in range(x.shape[0]):
        live = I[q] >= 0
        keys = key_of_id(I[q][live])
        _, first = np.unique(keys, return_index=True)
        first = np.sort(first)[:k]
        oD[q, :first.size], oI[q, :first.size], oG[q, :first.size] = D[q][live][first], I[q][live][first], keys[first]
    return oD, oI, oG


def _check_against_search(ix, X, ids, keys_of_rows, rng, ivf, nprobes=(None,)):
    N = ix.ntotal
    by_id = np.argsort(ids)
    key_of_id = lambda some: keys_of_rows[by_id[np.searchsorted(ids[by_id], some)]]
    ix.set_groups(ids, keys_of_rows)
    G = np.unique(keys_of_rows).size
    assert ix.ngroups == G
    P = SearchParametersIVF if ivf else SearchParameters
    lo, hi = int(np.sort(ids)[N // 5]), int(np.sort(ids)[N // 2])
    batch = ids[np.flatnonzero(keys_of_rows % 3 == 0)][::2]                        # two thirds of the groups lose all their rows
    alive = {IDSelectorRange: np.unique(keys_of_rows[(ids >= lo) & (ids < hi)]).size, IDSelectorBatch: np.unique(keys_of_rows[np.isin(ids, batch)]).size}
    assert 0 < alive[IDSelectorRange] < G and 0 < alive[IDSelectorBatch] < G
    selectors = (None, IDSelectorRange(lo, hi), IDSelectorBatch(batch))
    for nprobe in nprobes:
        for nq in (1, 3, 5):                                                        # passes of 4, 2 and 1 queries
            x = (X[rng.integers(0, N, nq)] + 0.25 * rng.standard_normal((nq, X.shape[1]))).astype(np.float32)
            x[0] = X[5]                                                             # its copies tie
            for sel in selectors:
                params = None if (sel is None and nprobe is None) else (P(sel=sel, nprobe=nprobe) if ivf else P(sel=sel))
                for k in (1, 10, G + 5):
                    got = ix.search_grouped(x, k, params=params)
                    want = _oracle(ix, x, k, key_of_id, params)
                    assert _same3(got, want), (nprobe, nq, type(sel).__name__, k)
                    if sel is not None and k > G:                                   # groups without a selected row do not appear
                        filled = (got[2] >= 0).sum(axis=1)
                        assert np.all(filled <= alive[type(sel)]) and (ivf or np.all(filled == alive[type(sel)]))


@pytest.mark.parametrize("d", [64, 512])
@pytest.mark.parametrize("name", ["IndexFlatIP", "IndexSQfp16", "IndexSQ8bit", "IndexFlatL2", "IndexSQfp16L2"])
def test_flat_types_against_search(name, d):
    N = 2000
    X, rng = _rows(N, d, 7)
    ids = np.arange(N, dtype=np.int64) * 3 + 7                                      # a range of ids is a range of rows: whole groups fall outside
    keys_of_rows = uneven_runs(rng, N, 60) * 5 + 2
    _check_against_search(_make_flat(name, d, X, ids), X, ids, keys_of_rows, rng, False)


@pytest.mark.parametrize("name", ["IndexIVFFlat", "IndexIVFSQ8", "IndexIVFSQfp16", "IndexIVFFlatL2"])
def test_ivf_types_against_search(name):
    N, d, nlist = 2000, 64, 16
    X, rng = _rows(N, d, 11)
    ids = np.arange(N, dtype=np.int64) * 3 + 7
    keys_of_rows = uneven_runs(rng, N, 60) * 5 + 2                                  # runs in add order: scattered over the lists
    _check_against_search(_make_ivf(name, d, nlist, X, ids), X, ids, keys_of_rows, rng, True, nprobes=(1, 4, 16))


# ---- (3) a grid of many blocks, against the restatements' scores
@pytest.fixture(scope="module")
def grid_data():
    rng = np.random.default_rng(3)
    N, d, nq = 50_000, 64, 3
    X = rng.standard_normal((N, d)).astype(np.float32)
    Q = (X[rng.integers(0, N, nq)] + 0.5 * rng.standard_normal((nq, d))).astype(np.float32)
    runs = uneven_runs(rng, N, 700)
    return X, Q, runs, rng.permutation(runs)


@pytest.mark.parametrize("name", ["IndexSQ8bit", "IndexFlatL2"])
def test_grid_of_many_blocks(name, grid_data):
    X, Q, runs, scattered = grid_data
    N = X.shape[0]
    ids = np.arange(N, dtype=np.int64) + 500
    ix = _make_flat(name, X.shape[1], X, ids)
    if name == "IndexSQ8bit":
        import sq8_flat_ref as ref
        vmin, vdiff = ix.trained_host()
        S = ref.scores(ix.rows_host()[0], vmin, vdiff, Q)
    else:
        import l2_flat_ref as ref
        S = ref.dists(X, Q)
    group_keys = np.arange(700, dtype=np.int64) + 9
    for gid in (runs, scattered):
        ix.set_groups(ids, group_keys[gid])
        for k in (10, 2048):
            got = ix.search_grouped(Q, k)
            want = gr.grouped(S, np.arange(N), gid, group_keys, k, None, ids, 0, ix.metric)
            assert _same3(got, want), k
        keep = (np.arange(N) % 7 != 0) & (gid % 4 != 1)                             # a quarter of the groups lose all their rows
        got = ix.search_grouped(Q, 100, params=SearchParameters(sel=IDSelectorBatch(ids[keep])))
        assert _same3(got, gr.grouped(S, np.arange(N), gid, group_keys, 100, keep, ids, 0, ix.metric))


# ---- (4) ties: the lower position wins, across groups and inside one, at block and segment boundaries
@pytest.mark.parametrize("name", ["IndexFlatIP", "IndexSQfp16", "IndexFlatL2"])
def test_ties_at_boundaries(name):
    N, d = 4200, 64
    rng = np.random.default_rng(5)
    X = (0.1 * rng.standard_normal((N, d))).astype(np.float32)
    star = rng.standard_normal(d).astype(np.float32)
    for r in (2047, 2048, 10, 4097):                                                # identical rows either side of row 2048, and far apart
        X[r] = star
    ids = np.arange(N, dtype=np.int64) * 2 + 1
    ix = _make_flat(name, d, X, ids)
    x = star[None, :].copy()
    gid = np.arange(N, dtype=np.int64) // 64 + 1000
    # the four copies in four groups: equal scores, ascending position
    ix.set_groups(ids, gid)
    D, I, G = ix.search_grouped(x, 4)
    assert I[0].tolist() == [ids[10], ids[2047], ids[2048], ids[4097]] and len(set(_bits(D)[0].tolist())) == 1
    assert G[0].tolist() == [gid[10], gid[2047], gid[2048], gid[4097]]
    # rows 2047 and 2048 in ONE group, and 10 and 4097 in another: each group is represented by its lower position
    two = gid.copy()
    two[2048] = two[2047]
    two[4097] = two[10]
    ix.set_groups(ids, two)
    D, I, G = ix.search_grouped(x, 3)
    assert I[0, :2].tolist() == [ids[10], ids[2047]] and G[0, :2].tolist() == [two[10], two[2047]] and _bits(D)[0, 0] == _bits(D)[0, 1]
    assert _bits(D)[0, 2] != _bits(D)[0, 0]


# ---- (5) argument errors: WISE_E_INVALID, the outputs untouched
def test_argument_errors_leave_outputs_untouched():
    lib = _lib.lib()
    N, G, nq, k, st = 300, 20, 2, 5, _lib.stream_ptr()
    rng = np.random.default_rng(8)
    gid = uneven_runs(rng, N, G)
    gid32, off, rows = tables_of(gid, G)
    d_ord = _dev((rng.integers(1, 9, size=(nq, N)) + 0x80000000).astype(np.uint32).view(np.int32))
    d_off, d_rows, d_gid, d_keys = _dev(off), _dev(rows.view(np.int32)), _dev(gid32), _dev(np.arange(G, dtype=np.int64))
    best = torch.full((nq, G), 0x5555, dtype=torch.int64, device="cuda")
    outs = [torch.full((nq, k), 3.5, dtype=torch.float32, device="cuda"), torch.full((nq, k), 1234, dtype=torch.int64, device="cuda"),
            torch.full((nq, k), 4321, dtype=torch.int64, device="cuda")]
    ws = torch.empty(lib.wise_group_workspace_bytes(N, G, nq, 2048), dtype=torch.uint8, device="cuda")
    good_best = (d_ord.data_ptr(), N, nq, d_off.data_ptr(), d_rows.data_ptr(), G, best.data_ptr(), st)
    for at, val, word in ((1, 0xFFFFFFFF, b"N="), (1, -1, b"N="), (5, N + 1, b"G="), (2, 0, b"nq="), (2, 65536, b"nq="), (3, 0, b"null")):
        args = list(good_best)
        args[at] = val
        assert lib.wise_group_best(*args) == WISE_E_INVALID and word in lib.wise_last_error(), (at, val)
    torch.cuda.synchronize()
    assert bool((best == 0x5555).all())
    good_topk = (best.data_ptr(), G, nq, k, d_gid.data_ptr(), N, d_keys.data_ptr(), 0, 0, 0, outs[0].data_ptr(), outs[1].data_ptr(),
                 outs[2].data_ptr(), ws.data_ptr(), ws.numel(), st)
    for at, val, word in ((3, 0, b"k="), (3, 2049, b"k="), (1, N + 1, b"G="), (2, 0, b"nq="), (5, 0xFFFFFFFF, b"N="), (12, 0, b"null"),
                          (14, 16, b"workspace"), (13, 0, b"workspace")):
        args = list(good_topk)
        args[at] = val
        assert lib.wise_group_topk(*args) == WISE_E_INVALID and word in lib.wise_last_error(), (at, val)
    X = _dev(rng.standard_normal((N, 64)).astype(np.float32))
    d_out = torch.full((nq, N), 7, dtype=torch.int32, device="cuda")
    assert lib.wise_ip_group_scores_f32(X.data_ptr(), N, 66, X.data_ptr(), nq, 0, d_out.data_ptr(), st) == WISE_E_INVALID
    assert lib.wise_l2_group_scores_f32(X.data_ptr(), N, 72, X.data_ptr(), nq, 0, d_out.data_ptr(), st) == WISE_E_INVALID
    assert lib.wise_ipsq16_group_scores(X.data_ptr(), N, 64, X.data_ptr(), 0, 0, d_out.data_ptr(), st) == WISE_E_INVALID
    assert lib.wise_ivfl2_group_scores(X.data_ptr(), N, 64, d_off.data_ptr(), 4, X.data_ptr(), nq, d_off.data_ptr(), 2049, 0, d_out.data_ptr(),
                                       st) == WISE_E_INVALID
    torch.cuda.synchronize()
    assert bool((outs[0] == 3.5).all()) and bool((outs[1] == 1234).all()) and bool((outs[2] == 4321).all()) and bool((d_out == 7).all())
    for bad in ((N, N + 1, 1, 1), (0xFFFFFFFF, 1, 1, 1), (N, G, 0, 1), (N, G, 1, 0), (N, G, 1, 2049), (-1, 0, 1, 1)):
        assert lib.wise_group_workspace_bytes(*bad) == 0, bad
    # and the same calls with good arguments work
    _lib.check(lib.wise_group_best(*good_best), "wise_group_best")
    _lib.check(lib.wise_group_topk(*good_topk), "wise_group_topk")
    want = gr.select(gr.best_keys(d_ord.cpu().numpy().view(np.uint32), gid, G), k, gid, np.arange(G))
    assert _same3(outs, want)


# ---- (6) staleness
def test_stale_groups_raise():
    from wise_amd.index.flat_sq import FlatSQfp16IPIndex
    rng = np.random.default_rng(9)
    X = rng.standard_normal((300, 64)).astype(np.float32)
    ix = FlatSQfp16IPIndex(64)
    with pytest.raises(RuntimeError, match="set_groups"):
        ix.search_grouped(X[:1], 3)
    ix.set_groups([], [])                                                           # no rows, no groups: padding
    D, I, G = ix.search_grouped(X[:2], 3)
    assert ix.ngroups == 0 and np.all(D == np.float32(-3.4028234663852886e38)) and np.all(I == -1) and np.all(G == -1)
    ix.add_with_ids(X, np.arange(300))
    ix.set_groups(np.arange(300), np.arange(300) // 10)
    D, I, G = ix.search_grouped(X[:2], 3)
    assert I[:, 0].tolist() == [0, 1] and G[:, 0].tolist() == [0, 0] and ix.ngroups == 30
    ix.add_with_ids(X[:5], np.arange(300, 305))
    with pytest.raises(RuntimeError, match="set_groups"):
        ix.search_grouped(X[:1], 3)
    ix.set_groups(np.arange(305), np.arange(305) // 10)
    assert ix.search_grouped(X[:1], 3)[1][0, 0] == 0
    assert ix.remove_ids(np.array([0, 1])) == 2
    assert ix.ngroups == 0
    with pytest.raises(RuntimeError, match="set_groups"):
        ix.search_grouped(X[:1], 3)
    ix.set_groups(np.arange(305), np.arange(305) // 10)                             # extra ids (the removed ones) are ignored
    assert ix.search_grouped(X[2:3], 2)[1][0, 0] == 2

"""-m gpu: IndexIVFFlatL2 — wise_l2_half_norms, wise_ivf_l2_coarse, wise_ivf_list_means and wise_ivfl2_scan(_sel),
wise_ivfl2_range_* through the C ABI against the numpy restatement (tests/ivf_l2_ref.py), bit for bit, then the index class, its
trainer, selectors, range_search, remove_ids and the SearchIndexFactory path on top of them."""
import os
import struct

import numpy as np
import pytest
import torch

import ivf_l2_ref as ref
import l2_flat_ref
from wise_amd import _lib
from wise_amd.index import faiss_io
from wise_amd.index.flat_l2 import FlatL2Index
from wise_amd.index.ivf_flat import IVFFlatL2Index, reference_nlist
from wise_amd.index.selector import IDSelectorBatch, IDSelectorNot, IDSelectorRange, SearchParametersIVF

pytestmark = pytest.mark.gpu

WISE_E_INVALID = -1
PAD = ref.PAD


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def keep_words(keep):
    """bool [N] -> uint32 words, bit (p & 31) of word p >> 5 (what wise_sel_bitmap writes), as int32 for torch"""
    n = len(keep)
    padded = np.zeros((n + 31) // 32 * 32, dtype=np.uint8)
    padded[:n] = keep
    return np.packbits(padded, bitorder="little").view(np.int32)


# ------------------------------------------------------------------------------------------------------------------ the coarse stage
def gpu_half_norms(C):
    C_d = dev(C)
    half = torch.full((C.shape[0],), 7.0, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().wise_l2_half_norms(C_d.data_ptr(), C.shape[0], C.shape[1], half.data_ptr(), _lib.stream_ptr()), "half_norms")
    return half


def gpu_coarse(X, C):
    """g [n, nlist] on the device: wise_ip_scores_f32, then wise_ivf_l2_coarse"""
    lib, st = _lib.lib(), _lib.stream_ptr()
    X_d, C_d, half = dev(X), dev(C), gpu_half_norms(C)
    G = torch.empty(X.shape[0], C.shape[0], dtype=torch.float32, device="cuda")
    _lib.check(lib.wise_ip_scores_f32(C_d.data_ptr(), C.shape[0], C.shape[1], X_d.data_ptr(), X.shape[0], G.data_ptr(), st), "scores")
    _lib.check(lib.wise_ivf_l2_coarse(G.data_ptr(), half.data_ptr(), X.shape[0], C.shape[0], st), "coarse")
    return G


@pytest.mark.parametrize("d", [16, 48, 512, 1024])
def test_half_norms_are_the_restatements_and_the_flat_index_ones(d):
    X = ref.long_rows(301, d, d)
    got = gpu_half_norms(X).cpu().numpy()
    assert np.array_equal(bits(got), bits(l2_flat_ref.half_norms(X)))
    lib, st = _lib.lib(), _lib.stream_ptr()
    X_d = dev(X)
    Xb = torch.empty(301, d, dtype=torch.int16, device="cuda")
    half = torch.empty(301, dtype=torch.float32, device="cuda")
    norms = torch.zeros(2, dtype=torch.float32, device="cuda")
    _lib.check(lib.wise_l2_prepare(X_d.data_ptr(), 301, d, Xb.data_ptr(), half.data_ptr(), norms.data_ptr(), st), "prepare")
    assert np.array_equal(bits(half.cpu().numpy()), bits(got))               # exactly wise_l2_prepare's
    h = torch.full((4,), 7.0, device="cuda")
    assert lib.wise_l2_half_norms(X_d.data_ptr(), 4, 24, h.data_ptr(), st) == WISE_E_INVALID and b"d=24" in lib.wise_last_error()
    assert lib.wise_l2_half_norms(X_d.data_ptr() + 4, 4, d, h.data_ptr(), st) == WISE_E_INVALID and b"aligned" in lib.wise_last_error()
    torch.cuda.synchronize()
    assert (h.cpu().numpy() == 7.0).all()


@pytest.mark.parametrize("d,nlist", [(16, 5), (48, 37), (128, 200)])
def test_coarse_rule_argmax_and_select(d, nlist):
    """g, the assignment and the probes are the restatement's; duplicate centroids: the lower list wins; nprobe > nlist pads with -1"""
    lib, st = _lib.lib(), _lib.stream_ptr()
    C = ref.long_rows(nlist, d, 3 * d, spread=3.0)
    C[nlist - 1] = C[1]                                              # equal centroids: equal g, the lower list takes the rows
    X = np.concatenate([ref.long_rows(130, d, d + 1), C[[1, 2]]])   # (rows that ARE centroids: nearest to themselves)
    G = gpu_coarse(X, C)
    want = ref.coarse_scores(X, C)
    assert np.array_equal(bits(G.cpu().numpy()), bits(want))
    a = torch.empty(X.shape[0], dtype=torch.int64, device="cuda")
    _lib.check(lib.wise_ivf_argmax(G.data_ptr(), X.shape[0], nlist, a.data_ptr(), st), "argmax")
    a = a.cpu().numpy()
    assert np.array_equal(a, ref.assign(X, C, G=want))
    assert a[130] == 1 and a[131] == 2 and not (a == nlist - 1).any()
    for nprobe in (1, 8, nlist, nlist + 9):
        P = torch.full((X.shape[0], nprobe), 7, dtype=torch.int64, device="cuda")
        _lib.check(lib.wise_select_topk_f32(G.data_ptr(), X.shape[0], nlist, nprobe, P.data_ptr(), st), "select")
        P = P.cpu().numpy()
        assert np.array_equal(P, ref.probes(X, C, nprobe, G=want)), nprobe
        assert (P == a[:, None]).any(axis=1).all()                   # a row's own list is among its probes at every nprobe
        if nprobe > nlist:
            assert (P[:, nlist:] == -1).all() and (P[:, :nlist] == np.arange(nlist)).all()


def test_list_means_divide_once_and_leave_empty_cells_alone():
    lib, st = _lib.lib(), _lib.stream_ptr()
    nlist, d = 9, 48
    rng = np.random.default_rng(4)
    sums = (rng.standard_normal((nlist, d)) * 50).astype(np.float32)
    counts = np.array([3, 0, 7, 1, 1000003, 0, 11, 13, 49], dtype=np.int64)
    want = ref.list_means(sums, counts)
    assert np.array_equal(bits(want[[1, 5]]), bits(sums[[1, 5]]))
    s_d, c_d = dev(sums), dev(counts)
    out = torch.full((nlist, d), 7.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.wise_ivf_list_means(s_d.data_ptr(), c_d.data_ptr(), nlist, d, out.data_ptr(), st), "means")
    got = out.cpu().numpy()
    full = counts > 0
    assert np.array_equal(bits(got[full]), bits(want[full])) and (got[~full] == 7.0).all()
    _lib.check(lib.wise_ivf_list_means(s_d.data_ptr(), c_d.data_ptr(), nlist, d, s_d.data_ptr(), st), "means in place")
    assert np.array_equal(bits(s_d.cpu().numpy()), bits(want))


# ------------------------------------------------------------------------------------------------------------------ the scan
NLIST, N = 37, 6000


class Case:
    """N = 6000 rows of lengths spread over 4x in 37 lists: empty lists, sizes from 1 row to many hundreds; equal rows within a list
    and in two lists; ids a permutation."""

    def __init__(self, d):
        rng = np.random.default_rng(200 + d)
        w = rng.uniform(0.2, 3.0, NLIST)
        w[[3, 20, 30]] = np.maximum(w[[3, 20, 30]], 1.0)             # (the lists that take the equal rows below: room for them)
        w[12], w[13] = 8.0, 0.2                                      # a long list and a short one
        w[[0, 9, 36]] = 0                                            # empty lists, the first and the last among them
        sizes = np.floor(w / w.sum() * (N - 40)).astype(np.int64)
        sizes[5] = 1
        sizes[20] += N - sizes.sum()
        full = np.sort(sizes[sizes > 0])
        assert sizes.sum() == N and full[0] == 1 and full[-1] > 2 * full[len(full) // 2] > 4 * full[1]    # sizes differ by more than 2x
        self.list_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        X = ref.long_rows(N, d, 300 + d)
        lo, hi = int(self.list_off[20]), int(self.list_off[21])
        X[hi - 5:hi - 2] = X[lo + 12:lo + 15]                        # equal rows within one list
        a, b = int(self.list_off[3]), int(self.list_off[30])
        X[b:b + 20] = X[a:a + 20]                                    # and in two lists
        norms = np.linalg.norm(X.astype(np.float64), axis=1)
        assert norms.max() / norms.min() >= 3.5                      # not normalised
        self.X, self.d = X, d
        self.ids = rng.permutation(N).astype(np.int64) * 7 + 1
        self.Q = (X[[lo + 13, a + 3, 17, 4000, 5999]] + np.float32(0.05) * ref.long_rows(5, d, 9, spread=1.0)).astype(np.float32)
        self.S = l2_flat_ref.dists(X, self.Q)                        # the restatement's distances, computed once
        self.X_d, self.off_d, self.ids_d, self.Q_d = dev(X), dev(self.list_off), dev(self.ids), dev(self.Q)

    def probe_sets(self, nq):
        """nprobe -> [nq, nprobe]: 1: an empty list, the list of one row, a long list; 8: with -1, a value >= nlist and a list named
        twice; 64 (more than nlist): every list once, then -1, out-of-range values and a repeat"""
        rng = np.random.default_rng(5)
        one = np.array([[9], [5], [20], [3], [30]], dtype=np.int64)[:nq]
        eight = np.stack([rng.permutation(NLIST)[:8] for _ in range(nq)]).astype(np.int64)
        eight[:, 2], eight[:, 5], eight[:, 6] = -1, NLIST + 3, eight[:, 0]
        wide = np.full((nq, 64), -1, dtype=np.int64)
        for q in range(nq):
            wide[q, rng.permutation(64)[:NLIST]] = rng.permutation(NLIST)
            free = np.flatnonzero(wide[q] == -1)
            wide[q, free[0]], wide[q, free[1]], wide[q, free[2]] = NLIST, 1 << 40, 20
        return {1: one, 8: eight, 64: wide}

    def raw_scan(self, nq, probes_d, k, with_ids=True, keep_d=None, sel=False, ws_bytes=None, d=None, X_ptr=None):
        lib = _lib.lib()
        nprobe = probes_d.shape[1]
        need = lib.wise_ivfl2_scan_workspace_bytes(nq, nprobe, k)
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
        D = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
        I = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
        head = (self.X_d.data_ptr() if X_ptr is None else X_ptr, N, self.d if d is None else d, self.off_d.data_ptr(), NLIST,
                self.ids_d.data_ptr() if with_ids else 0, self.Q_d.data_ptr(), nq, probes_d.data_ptr(), nprobe, k)
        tail = (D.data_ptr(), I.data_ptr(), ws.data_ptr(), need if ws_bytes is None else ws_bytes, _lib.stream_ptr())
        if sel:
            rc = lib.wise_ivfl2_scan_sel(*head, 0 if keep_d is None else keep_d.data_ptr(), *tail)
        else:
            rc = lib.wise_ivfl2_scan(*head, *tail)
        return rc, D, I

    def scan(self, nq, probes_d, k, with_ids=True, keep_d=None):
        rc, D, I = self.raw_scan(nq, probes_d, k, with_ids, keep_d, sel=keep_d is not None)
        _lib.check(rc, "wise_ivfl2_scan")
        return D.cpu().numpy(), I.cpu().numpy()


_CASES = {}


def case_of(d):
    if d not in _CASES:
        _CASES[d] = Case(d)
    return _CASES[d]


def prefix(Dfull, Ifull, k):
    return np.ascontiguousarray(Dfull[:, :k]), np.ascontiguousarray(Ifull[:, :k])


@pytest.mark.parametrize("d", [16, 48, 512, 1024])
def test_scan_is_bit_equal_to_the_restatement(d):
    case = case_of(d)
    for nq in (1, 5):
        for nprobe, probes in case.probe_sets(nq).items():
            probes_d = dev(probes)
            for with_ids in (True, False):
                Dfull, Ifull = ref.scan(case.X, case.list_off, case.ids if with_ids else None, case.Q[:nq], probes, 100, S=case.S[:nq])
                for k in (1, 10, 100):
                    D, I = case.scan(nq, probes_d, k, with_ids)
                    Do, Io = prefix(Dfull, Ifull, k)
                    what = f"d={d} nq={nq} nprobe={nprobe} k={k} ids={with_ids}"
                    assert np.array_equal(bits(D), bits(Do)), what
                    assert np.array_equal(I, Io), what
            if nprobe == 1:                                          # an empty list, and the list of one row: padding
                assert (Ifull[0] == -1).all() and (Dfull[0] == PAD).all()
                if nq == 5:
                    assert Ifull[1, 0] >= 0 and (Ifull[1, 1:] == -1).all() and (Dfull[1, 1:] == PAD).all()
    # every list probed: a row's distance is IndexFlatL2's, the equal rows tie and the lower position wins, within a list and across
    probes = np.tile(np.arange(NLIST, dtype=np.int64), (5, 1))
    D, I = case.scan(5, dev(probes), 100, with_ids=False)
    Df, If = l2_flat_ref.topk(case.X, case.Q, 100, S=case.S)
    assert np.array_equal(bits(D), bits(Df)) and np.array_equal(I, If)
    lo, a, b = int(case.list_off[20]), int(case.list_off[3]), int(case.list_off[30])
    hi = int(case.list_off[21])
    assert I[0, 0] == lo + 13 and I[0, 1] == hi - 4 and bits(D[0, 0]) == bits(D[0, 1])
    assert I[1, 0] == a + 3 and I[1, 1] == b + 3 and bits(D[1, 0]) == bits(D[1, 1])


def test_selector_scan():
    case = case_of(48)
    nq = 5
    probes = case.probe_sets(nq)[64]
    probes_d = dev(probes)
    rng = np.random.default_rng(1)
    Dp, Ip = case.scan(nq, probes_d, 100)
    for name, keep in (("empty", np.zeros(N, bool)), ("random", rng.random(N) < 0.5), ("sparse", rng.random(N) < 0.01), ("all", np.ones(N, bool))):
        keep_d = dev(keep_words(keep))
        for k in (1, 10, 100):
            Do, Io = ref.scan(case.X, case.list_off, case.ids, case.Q, probes, k, keep=keep, S=case.S)
            D, I = case.scan(nq, probes_d, k, keep_d=keep_d)
            assert np.array_equal(bits(D), bits(Do)) and np.array_equal(I, Io), (name, k)
        if name == "empty":
            assert (I == -1).all() and (D == PAD).all()
        if name == "all":
            assert np.array_equal(bits(D), bits(Dp)) and np.array_equal(I, Ip)
        if name == "sparse":                                         # a selected row's distance is the unfiltered scan's
            pos_of = {int(i): p for p, i in enumerate(case.ids)}
            for q in range(nq):
                for dd, i in zip(D[q], I[q]):
                    assert i == -1 or bits(dd) == bits(case.S[q, pos_of[int(i)]])


def test_bad_arguments_are_refused_and_nothing_is_written():
    case = case_of(48)
    lib = _lib.lib()
    probes_d = dev(case.probe_sets(2)[8])
    need = lib.wise_ivfl2_scan_workspace_bytes(2, 8, 10)
    assert need > 0 and lib.wise_ivfl2_scan_workspace_bytes(2, 2049, 10) == 0 and lib.wise_ivfl2_scan_workspace_bytes(2, 8, 2049) == 0
    keep_d = dev(keep_words(np.ones(N, bool)))
    for sel in (False, True):
        for kw, what in ((dict(d=24), b"d=24"), (dict(d=1040), b"d=1040"), (dict(ws_bytes=need - 1), b"workspace"),
                         (dict(X_ptr=case.X_d.data_ptr() + 4), b"16-byte aligned")):
            rc, D, I = case.raw_scan(2, probes_d, 10, keep_d=keep_d if sel else None, sel=sel, **kw)
            assert rc == WISE_E_INVALID and what in lib.wise_last_error(), (what, lib.wise_last_error())
            torch.cuda.synchronize()
            assert (D.cpu().numpy() == 7.0).all() and (I.cpu().numpy() == 7).all()      # nothing ran: the outputs are untouched
    rc, D, I = case.raw_scan(2, probes_d, 10, keep_d=None, sel=True)
    assert rc == WISE_E_INVALID and b"null bitmap" in lib.wise_last_error()
    torch.cuda.synchronize()
    assert (D.cpu().numpy() == 7.0).all() and (I.cpu().numpy() == 7).all()
    st = _lib.stream_ptr()
    q = case.Q_d.data_ptr()
    for fn, args in ((lib.wise_ivfl2_range_count, (0.5, 0, 0)), (lib.wise_ivfl2_range_fill, (0.5, 0, 0, 0))):
        head = (case.X_d.data_ptr(), N, 24, case.off_d.data_ptr(), NLIST) + ((0,) if fn is lib.wise_ivfl2_range_fill else ())
        assert fn(*head, q, 2, probes_d.data_ptr(), 8, *args, q, 1 << 20, st) == WISE_E_INVALID
        assert b"d=24" in lib.wise_last_error()


# ------------------------------------------------------------------------------------------------------------------ range_search
@pytest.mark.parametrize("with_keep", [False, True])
def test_range_count_and_fill(with_keep):
    """radii that return no row (the smallest distance itself: strictly less), some rows and every row of the probed lists; the
    hits come in probe order, then by ascending position, with the scan's distances"""
    lib, st = _lib.lib(), _lib.stream_ptr()
    case = case_of(48)
    nq = 5
    rng = np.random.default_rng(8)
    probes = np.stack([rng.permutation(NLIST)[:8] for _ in range(nq)]).astype(np.int64)
    probes[:, 3], probes[:, 6] = -1, NLIST + 1
    keep = rng.random(N) < 0.4 if with_keep else None
    keep_d = dev(keep_words(keep)) if with_keep else None
    cand = [ref.candidates(case.list_off, probes[q], keep) for q in range(nq)]
    assert all(len(c) > 100 for c in cand)
    t_none = float(min(case.S[q, cand[q]].min() for q in range(nq)))
    t_some = float(np.median(np.concatenate([case.S[q, cand[q]] for q in range(nq)])))
    t_all = float(max(case.S[q, cand[q]].max() for q in range(nq))) * 2.0
    probes_d = dev(probes)
    need = lib.wise_ivfl2_range_workspace_bytes(N, NLIST, nq, 8)
    assert need > 0
    head = (case.X_d.data_ptr(), N, 48, case.off_d.data_ptr(), NLIST)
    mid = (case.Q_d.data_ptr(), nq, probes_d.data_ptr(), 8)
    for t, kind in ((t_none, "none"), (t_some, "some"), (t_all, "all")):
        lims, Dw, Pw = ref.range_raw(case.X, case.list_off, case.Q, probes, t, keep, S=case.S)
        n = np.diff(lims)
        assert (kind != "none" or (n == 0).all()) and (kind != "all" or (n == [len(c) for c in cand]).all())
        assert kind != "some" or (0 < n.sum() < sum(len(c) for c in cand))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        counts = torch.full((nq,), -7, dtype=torch.int64, device="cuda")
        _lib.check(lib.wise_ivfl2_range_count(*head, *mid, t, _lib.ptr(keep_d), counts.data_ptr(), ws.data_ptr(), need, st), "count")
        assert np.array_equal(counts.cpu().numpy(), n), kind
        total = int(lims[-1])
        lims_d = dev(lims)
        for with_ids in (True, False):
            D = torch.full((total + 1,), 7.5, dtype=torch.float32, device="cuda")
            I = torch.full((total + 1,), -99, dtype=torch.int64, device="cuda")
            _lib.check(lib.wise_ivfl2_range_fill(*head, case.ids_d.data_ptr() if with_ids else 0, *mid, t, lims_d.data_ptr(), D.data_ptr(),
                                                 I.data_ptr(), ws.data_ptr(), need, st), "fill")
            D, I = D.cpu().numpy(), I.cpu().numpy()
            assert D[total] == 7.5 and I[total] == -99                # nothing written past lims[nq]
            assert np.array_equal(bits(D[:total]), bits(Dw)) and np.array_equal(I[:total], case.ids[Pw] if with_ids else Pw), (kind, with_ids)


# ------------------------------------------------------------------------------------------------------------------ the index
TN, TD, TNLIST = 2000, 32, 16


@pytest.fixture(scope="module")
def built():
    """2000 x 32 clustered rows of lengths spread over 4x in 16 lists: (X, ids, index trained with niter 3 and filled in one add, the
    restated trainer's centroids)"""
    X = ref.long_rows(TN, TD, 21, centres=12)
    ids = np.random.default_rng(2).permutation(TN).astype(np.int64) * 2 + 5
    idx = IVFFlatL2Index(TD, TNLIST)
    idx.niter = 3
    assert not idx.is_trained and idx.metric == "l2"
    idx.train(X)
    assert idx.is_trained
    idx.add_with_ids(X, ids)
    return X, ids, idx, ref.train(X, TNLIST, niter=3)


def index_reference(idx, Q, k, nprobe, keep=None):
    """the restatement on the index's own centroids and lists"""
    c, Xs, ids_s, off = idx.lists_host()
    return ref.scan(Xs, off, ids_s, Q, ref.probes(Q, c, nprobe), k, keep=keep)


def test_training_is_deterministic_and_the_restated_trainer(built):
    X, ids, idx, C = built
    c = idx.lists_host()[0]
    assert np.array_equal(bits(c), bits(C))
    again = IVFFlatL2Index(TD, TNLIST)
    again.niter = 3
    again.train(X)
    assert np.array_equal(bits(again.centroids.cpu().numpy()), bits(c))
    norms = np.linalg.norm(c.astype(np.float64), axis=1)
    assert norms.max() / norms.min() > 1.2                          # means, not unit vectors
    assert np.array_equal(idx.assign(X), ref.assign(X, c))
    probes = idx.probes_device(dev(X[:50]), 5).cpu().numpy()
    assert np.array_equal(probes, ref.probes(X[:50], c, 5))
    with pytest.raises(ValueError):
        IVFFlatL2Index(40, 4)
    with pytest.raises(RuntimeError):
        IVFFlatL2Index(TD, 4).add_with_ids(X[:4], ids[:4])
    with pytest.raises(ValueError):
        IVFFlatL2Index(TD, 64).train(X[:10])


def test_index_chunked_adds_and_state(built):
    X, ids, idx, C = built
    c, Xs, ids_s, off = idx.lists_host()
    order, list_off = ref.build(X, c)
    assert np.array_equal(off, list_off) and np.array_equal(ids_s, ids[order]) and np.array_equal(bits(Xs), bits(X[order]))
    st = idx.state_host()
    assert set(st) == {"centroids", "X", "ids", "list_off", "nprobe", "metric"} and st["metric"] == "l2" and idx.ntotal == TN
    idx2 = IVFFlatL2Index(TD, TNLIST)
    idx2.set_centroids(c)
    assert idx2.is_trained
    for s, e in ((0, 700), (700, 701), (701, TN)):                  # chunks give the same lists as one add
        idx2.add_with_ids(X[s:e], ids[s:e])
    for u, v in zip(idx.lists_host(), idx2.lists_host()):
        assert u.tobytes() == v.tobytes()


def test_index_search_flat_equality_selectors_and_reconstruct(built):
    X, ids, idx, C = built
    Q = (X[:9] + np.float32(0.05) * ref.long_rows(9, TD, 4, spread=1.0)).astype(np.float32)
    c, Xs, ids_s, off = idx.lists_host()
    for nprobe, k in ((1, 10), (4, 100), (16, 10)):
        idx.nprobe = nprobe
        D, I = idx.search(Q, k)
        Do, Io = index_reference(idx, Q, k, nprobe)
        assert np.array_equal(bits(D), bits(Do)) and np.array_equal(I, Io), (nprobe, k)
        assert (np.diff(D.astype(np.float64), axis=1) >= 0).all()    # squared distances, ascending
    assert (I[:, 0] == ids[:9]).all()
    # nprobe = nlist: IndexFlatL2 over the same rows, distances bit for bit; no equal distances among the first k + 1 of the
    # restatement, so the id sets agree too
    flat = FlatL2Index(TD)
    flat.add_with_ids(X, ids)
    Df, If = flat.search(Q, 10)
    S = l2_flat_ref.dists(X, Q)
    first = np.sort(S, axis=1)[:, :11]
    assert (np.diff(first, axis=1) > 0).all()
    assert np.array_equal(bits(D), bits(Df)) and all(set(I[q]) == set(If[q]) for q in range(9)) and np.array_equal(I, If)
    # L2 and the inner product order the top 10 differently on rows that are not normalised
    ip = (Q.astype(np.float64) @ X.astype(np.float64).T)
    top_ip = np.argsort(-ip, axis=1, kind="stable")[:, :10]
    top_l2 = np.argsort(S.astype(np.float64), axis=1, kind="stable")[:, :10]
    assert any(set(top_ip[q]) != set(top_l2[q]) for q in range(9))
    assert np.array_equal(I, ids[top_l2])
    idx.make_direct_map(True)
    rec = idx.reconstruct_batch([int(ids_s[0]), int(ids_s[TN - 1]), 4, int(ids_s[777])])
    assert np.array_equal(bits(rec[[0, 1, 3]]), bits(Xs[[0, TN - 1, 777]])) and np.isnan(rec[2]).all()
    some = np.sort(ids[np.random.default_rng(3).permutation(TN)[:200]])
    for sel, kept in ((IDSelectorBatch(some), np.isin(ids_s, some)),
                      (IDSelectorRange(1000, 3000), (ids_s >= 1000) & (ids_s < 3000)),
                      (IDSelectorNot(IDSelectorBatch(some)), ~np.isin(ids_s, some))):
        D, I = idx.search(Q, 10, params=SearchParametersIVF(sel=sel, nprobe=5))
        Do, Io = index_reference(idx, Q, 10, 5, keep=kept)
        assert np.array_equal(bits(D), bits(Do)) and np.array_equal(I, Io)
        assert np.isin(I[I >= 0], ids_s[kept]).all()
    assert idx.nprobe == 16                                          # the parameter's nprobe held for that call only


def test_index_range_search(built):
    X, ids, idx, C = built
    Q = (X[[3, 500, 999, 1500]] + np.float32(0.01)).astype(np.float32)
    c, Xs, ids_s, off = idx.lists_host()
    idx.nprobe = 6
    probes = ref.probes(Q, c, 6)
    S = l2_flat_ref.dists(Xs, Q)
    t = float(np.sort(np.concatenate([S[q, ref.candidates(off, probes[q])] for q in range(4)]))[150])
    lims, D, I = idx.range_search(Q, t)
    wl, wD, wI = ref.range_search(Xs, off, ids_s, Q, probes, t, S=S)
    assert lims.dtype == np.int64 and np.array_equal(lims, wl) and lims[-1] == 150
    assert np.array_equal(bits(D), bits(wD)) and np.array_equal(I, wI)
    for q in range(4):
        assert (np.diff(D[lims[q]:lims[q + 1]].astype(np.float64)) >= 0).all() and (D[lims[q]:lims[q + 1]] < np.float32(t)).all()
    qd = dev(Q)
    whole = idx.range_search_device(qd, t)
    cut = idx.range_search_device(qd, t, chunk=3)
    assert torch.equal(whole[0], cut[0]) and torch.equal(whole[1].view(torch.int32), cut[1].view(torch.int32)) and torch.equal(whole[2], cut[2])
    some = np.sort(ids[np.random.default_rng(3).permutation(TN)[:TN // 3]])
    ls, Ds, Is = idx.range_search(Q, t, params=SearchParametersIVF(sel=IDSelectorBatch(some)))
    wl, wD, wI = ref.range_search(Xs, off, ids_s, Q, probes, t, keep=np.isin(ids_s, some), S=S)
    assert np.array_equal(ls, wl) and np.array_equal(bits(Ds), bits(wD)) and np.array_equal(Is, wI)
    l0, D0, I0 = idx.range_search(Q, 0.0)
    assert l0.tolist() == [0] * 5 and D0.shape == (0,) and I0.shape == (0,)
    l1, _, _ = idx.range_search(Q, t, params=SearchParametersIVF(nprobe=16))
    assert idx.nprobe == 6 and (np.diff(l1) >= np.diff(lims)).all()
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            idx.range_search(Q, bad)
    idx.nprobe = 16


def test_remove_ids_leaves_the_index_of_the_kept_rows(built):
    X, ids, idx0, C = built
    c = idx0.lists_host()[0]
    gone = np.random.default_rng(8).random(TN) < 0.3
    a, b = IVFFlatL2Index(TD, TNLIST), IVFFlatL2Index(TD, TNLIST)
    for i in (a, b):
        i.set_centroids(c)
    a.add_with_ids(X, ids)
    assert a.remove_ids(ids[gone], scratch_bytes=100 * 1024) == int(gone.sum())
    b.add_with_ids(X[~gone], ids[~gone])
    for u, v in zip(a.lists_host(), b.lists_host()):
        assert u.shape == v.shape and u.tobytes() == v.tobytes()
    assert a.ntotal == int((~gone).sum())
    a.nprobe = b.nprobe = 5
    Da, Ia = a.search(X[:4], 10)
    Db, Ib = b.search(X[:4], 10)
    assert np.array_equal(bits(Da), bits(Db)) and np.array_equal(Ia, Ib) and not np.isin(Ia, ids[gone]).any()
    assert np.isnan(a.reconstruct_batch([int(ids[gone][0])])).all()


# ------------------------------------------------------------------------------------------------------------------ the plugin
def write_shard(fdir, first_shard, ids, rows):
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    st = FeatureStoreFactory.create_store(FeatureStoreType.WEBDATASET, "video", str(fdir))
    st.enable_write(1024, 20 * 1024 * 1024, first_shard=first_shard)
    for i, r in zip(ids, rows):
        st.add(int(i), r[None, :])
    st.close()


def test_plugin_builds_loads_filters_ranges_and_updates(tmp_path):
    from wise_amd.index.search_index_factory import SearchIndexFactory

    fdir, idir = tmp_path / "features", tmp_path / "index"
    fdir.mkdir()
    n, d, n_new = 3072, 64, 512
    ITYPE = "IndexIVFFlatL2"
    X = ref.long_rows(n + n_new, d, 21, centres=16)
    ids = np.arange(1, n + n_new + 1, dtype=np.int64)
    write_shard(fdir, 0, ids[:n], X[:n])
    si = SearchIndexFactory("video", "mlfoundations/open_clip/ViT-B-32/seeded-0", {"features_dir": fdir, "index_dir": idir})
    si.create_index(ITYPE)
    fn = si.get_index_filename(ITYPE)
    assert fn.name == "video-IndexIVFFlatL2.faiss" and faiss_io.index_fourcc(fn) == "IwFl" and faiss_io.ivf_flat_metric(fn) == 1
    raw = fn.read_bytes()
    assert struct.unpack_from("<i", raw, 4 + 29)[0] == 1 and raw[4 + 33 + 16:4 + 33 + 20] == b"IxF2"
    nlist = reference_nlist(n)
    # the same build by hand: the file holds its lists, and the loaded index gives its answers
    mine = IVFFlatL2Index(d, nlist)
    mine.train(X[:n][np.sort(np.random.default_rng(1234).permutation(n)[:min(n, 100 * nlist)])])
    mine.add_with_ids(X[:n], ids[:n])
    want_fn = tmp_path / "want.faiss"
    si._write_index_file(mine, want_fn)
    assert raw == want_fn.read_bytes()
    assert si.load_index(ITYPE) is True and type(si.index) is IVFFlatL2Index
    index = si.index
    assert index.nlist == nlist and index.ntotal == n and index.nprobe == 1
    index.nprobe = mine.nprobe = 8
    Q = X[:6]
    D, I = index.search(Q, 10)
    Dm, Im = mine.search(Q, 10)
    assert np.array_equal(bits(D), bits(Dm)) and np.array_equal(I, Im) and (I[:, 0] == np.arange(1, 7)).all() and (D[:, 0] == 0).all()
    index.nprobe = nlist

    class Words:                                                     # the text tower gives 512 dimensions; this store has 64
        def extract_text_features(self, texts):
            return np.stack([X[len(t)] + np.float32(0.01) for t in texts])

    si.feature_extractor = Words()
    within = np.arange(100, 130, dtype=np.int64)
    dist, got = si.search("video", "dog", topk=5, within=within)
    assert dist.shape == (5,) and np.isin(got, within).all() and len(set(got.tolist())) == 5 and np.all(np.diff(dist) >= 0)
    both = si.search_batch("video", ["dog", "a cat"], topk=50, within=within)
    for dd, i in both:
        assert set(i[:30].tolist()) == set(within.tolist()) and (i[30:] == -1).all() and (dd[30:] == PAD).all()
    top_d, top_i = si.search("video", "dog", topk=200)
    t = float(top_d[40])
    rd, ri = si.search_range("video", "dog", t)                      # a radius, as IndexFlatL2: dist < t, strictly
    m = top_d < np.float32(t)
    assert 1 <= len(rd) <= 40 and np.array_equal(bits(rd), bits(top_d[m])) and np.array_equal(ri, top_i[m])
    wide = np.arange(100, 900, dtype=np.int64)
    dw, iw = si.search_range("video", "dog", t, within=wide)
    m = np.isin(ri, wide)
    assert np.array_equal(iw, ri[m]) and np.array_equal(bits(dw), bits(rd[m]))
    del si.index, si.feature_extractor
    # update_index: the store loses its middle shard and gains a fourth
    write_shard(fdir, 3, ids[n:], X[n:])
    os.remove(fdir / "video-000001.tar")
    kept = np.concatenate([np.arange(0, 1024), np.arange(2048, n)])
    f = faiss_io.read_index(fn)
    assert f["metric"] == "l2"
    want = IVFFlatL2Index(d, nlist)
    want.set_centroids(f["centroids"])
    want.nprobe = f["nprobe"]
    want.add_with_ids(X[kept], ids[kept])
    want.add_with_ids(X[n:], ids[n:])
    si._write_index_file(want, want_fn)
    assert si.update_index(ITYPE) == (512, 1024)
    assert fn.read_bytes() == want_fn.read_bytes() and faiss_io.ivf_flat_metric(fn) == 1
    assert si.update_index(ITYPE) == (0, 0)
    assert si.load_index(ITYPE) is True and si.index.ntotal == 2048 + 512 and type(si.index) is IVFFlatL2Index

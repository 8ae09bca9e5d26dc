"""-m gpu: search restricted to a set of ids — the selector kernels and the SEL forms of the three scans through the C ABI and the
index classes, against the numpy restatement (tests/sel_ref.py)."""
import numpy as np
import pytest
import torch

import ivfpq_ref
import ivfpq_refine_ref as rr
import sel_ref
from oracle import ip_topk_ref
from wise_amd import _lib
from wise_amd.index.flat_ip import FlatIPIndex
from wise_amd.index.ivf_flat import IVFFlatIPIndex
from wise_amd.index.ivf_pq import IVFOPQIPIndex, IVFOPQRefineIPIndex, IVFPQIPIndex, IVFPQRefineIPIndex
from wise_amd.index.selector import (IDSelectorBatch, IDSelectorNot, IDSelectorRange, ResolvedSelector, SearchParameters,
                                     SearchParametersIVF)

pytestmark = pytest.mark.gpu

NEG = ip_topk_ref.NEG
TOL = 2e-5          # tests/test_gpu_ip_topk.py: check_against_oracle's tolerance on the scores


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_selector(kind, args):
    if kind == "range":
        return IDSelectorRange(*args)
    return IDSelectorBatch(*args) if kind == "batch" else IDSelectorNot(IDSelectorBatch(*args))


# ------------------------------------------------------------------------------------------------ wise_sel_bitmap / _positions
def gpu_bitmap(ids, id_base, N, selector):
    """(bitmap uint32 [ceil(N/32)], positions int64, count) through the C ABI; ids None: the id_base form"""
    lib, st = _lib.lib(), _lib.stream_ptr()
    mode, sorted_ids, imin, imax, invert = selector._spec(torch.device("cuda"))
    ids_d = None if ids is None else dev(ids)
    words = (N + 31) // 32
    bm = torch.full((words + 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")         # two guard words behind the bitmap
    _lib.check(lib.wise_sel_bitmap(_lib.ptr(ids_d), id_base, N, mode, _lib.ptr(sorted_ids), 0 if sorted_ids is None else sorted_ids.numel(),
                                   imin, imax, int(invert), bm.data_ptr(), st), "wise_sel_bitmap")
    assert (bm[words:] == 0x5A5A5A5A).all()                                            # nothing written past the last word
    pos = torch.full((N + 1,), -9, dtype=torch.int64, device="cuda")
    count = torch.full((1,), -9, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(lib.wise_sel_positions_workspace_bytes(N), 1), dtype=torch.uint8, device="cuda")
    _lib.check(lib.wise_sel_positions(bm.data_ptr(), N, pos.data_ptr(), N, count.data_ptr(), ws.data_ptr(), ws.numel(), st),
               "wise_sel_positions")
    n = int(count.item())
    assert 0 <= n <= N and (pos[n:] == -9).all()
    return bm[:words].cpu().numpy().view(np.uint32), pos[:n].cpu().numpy(), n


@pytest.mark.parametrize("N", [1, 31, 63, 64, 65, 1000, 8191, 8193, 100003, 2100001])
def test_bitmap_and_positions_equal_the_restatement(N):
    rng = np.random.default_rng(N)
    ids = rng.permutation(N).astype(np.int64) * 3 + 11
    some = rng.permutation(ids)[: max(N // 7, 1)]
    batch = IDSelectorBatch(np.concatenate([some, some[:5], [-3, 1, 10 ** 12]]))        # duplicates, ids no row carries
    selectors = [batch, IDSelectorBatch([]), IDSelectorRange(11, 11 + 3 * (N // 3)), IDSelectorRange(5, 5), IDSelectorRange(-1, 10 ** 15),
                 IDSelectorNot(batch), IDSelectorNot(IDSelectorRange(40, 40 + N)), IDSelectorNot(IDSelectorNot(batch)),
                 IDSelectorNot(IDSelectorBatch([]))]
    for sel in selectors:
        for form_ids, id_base in ((ids, 0), (None, 17)):
            row_ids = ids if form_ids is not None else np.arange(N, dtype=np.int64) + id_base
            mask = sel_ref.resolve(row_ids, sel)
            bm, pos, n = gpu_bitmap(form_ids, id_base, N, sel)
            assert np.array_equal(bm, sel_ref.bitmap(mask))                            # every word, the zero tail bits included
            assert n == int(mask.sum()) and np.array_equal(pos, np.flatnonzero(mask))  # ascending
            bm2, pos2, n2 = gpu_bitmap(form_ids, id_base, N, sel)
            assert np.array_equal(bm, bm2) and np.array_equal(pos, pos2) and n == n2   # identical on two runs
    # the position list is cut at `capacity`, the count is not
    lib, st = _lib.lib(), _lib.stream_ptr()
    bm_d = dev(sel_ref.bitmap(np.ones(N, bool)).view(np.int32))
    pos = torch.full((N + 1,), -9, dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.wise_sel_positions_workspace_bytes(N), dtype=torch.uint8, device="cuda")
    cap = N // 2
    _lib.check(lib.wise_sel_positions(bm_d.data_ptr(), N, pos.data_ptr(), cap, count.data_ptr(), ws.data_ptr(), ws.numel(), st), "positions")
    assert int(count.item()) == N and (pos[cap:] == -9).all() and torch.equal(pos[:cap].cpu(), torch.arange(cap))


def test_positions_over_more_blocks_than_one_scan_pass():
    """9M rows are 1099 blocks of 8192: the scan of the block counts takes a second pass of its 1024 threads."""
    N = 9_000_001
    for sel in (IDSelectorRange(5_000_000, 8_999_990), IDSelectorNot(IDSelectorRange(100, 8_500_000))):
        mask = sel_ref.resolve(np.arange(N, dtype=np.int64) + 3, sel)
        bm, pos, n = gpu_bitmap(None, 3, N, sel)
        assert np.array_equal(bm, sel_ref.bitmap(mask)) and n == int(mask.sum()) and np.array_equal(pos, np.flatnonzero(mask))


# ------------------------------------------------------------------------------------------------------------------------ flat
def check_flat(D, I, S64, mask, ids, k, what):
    """The filtered search against sel_ref.filtered_topk over the float64 scores: padding exact, scores within TOL (the
    comparison of tests/test_gpu_ip_topk.py), ids equal on every rank but the oracle's near-ties (sel_ref.NEAR_TIE), which may be
    at most 1 % of the compared ranks of the case."""
    nq = D.shape[0]
    Do, Io, _ = sel_ref.filtered_topk(S64[:nq], np.arange(S64.shape[1]), mask, ids, k)
    assert D.shape == Do.shape and I.shape == Io.shape and I.dtype == np.int64 and D.dtype == np.float32, what
    assert np.array_equal(I == -1, Io == -1), what                                     # padding in the tail only, where the oracle's is
    assert np.all(D[I == -1] == NEG), what
    valid = Io != -1
    assert np.allclose(D[valid], Do[valid], atol=TOL, rtol=0), (what, np.abs(D[valid] - Do[valid]).max())
    assert np.all(np.diff(D, axis=1) <= 0), what
    assert np.isin(I[valid], ids[mask]).all(), what                                    # no unselected id, ever
    near = sel_ref.near_tie_ranks(S64[:nq], mask, k)
    share = near.sum() / max(valid.sum(), 1)
    print(f"{what}: {int(valid.sum())} ranks compared, {int(near.sum())} near-ties left out ({100 * share:.2f} %), "
          f"max |dD| {np.abs(D[valid] - Do[valid]).max() if valid.any() else 0:.2e}")
    assert share <= 0.01, (what, share)
    assert np.array_equal(I[~near], Io[~near]), what


@pytest.mark.parametrize("d", [64, 512, 768])
@pytest.mark.parametrize("N", [1000, 4096, 300000])
def test_flat_filtered_search_equals_the_restatement(N, d):
    X, Q, ids = sel_ref.flat_case(N, d)
    S64 = sel_ref.scores_f64(X, Q)
    idx = FlatIPIndex(d)
    for s in range(0, N, 100000):
        idx.add_with_ids(X[s:s + 100000], ids[s:s + 100000])
    for which in sel_ref.SELECTIVITIES:
        sel = make_selector(*sel_ref.flat_selector_spec(ids, which))
        mask = sel_ref.resolve(ids, sel)
        assert {"all": N, "one": 1, "none": 0}.get(which, mask.sum()) == mask.sum()
        for nq in (1, 8):
            for k in (1, 10, 100):
                D, I = idx.search(Q[:nq], k, params=SearchParameters(sel=sel))
                check_flat(D, I, S64, mask, ids, k, f"N={N} d={d} {which} nq={nq} k={k}")
    assert idx.shadow_counts() == (0, 0)


def test_flat_exact_ties_go_to_the_lower_selected_position():
    """Small-integer rows and queries: every dot product is exact in fp32 in any order, and thousands of rows tie."""
    N, d = 4096, 64
    rng = np.random.default_rng(5)
    X = rng.integers(-1, 2, (N, d)).astype(np.float32)
    Q = rng.integers(-1, 2, (3, d)).astype(np.float32)
    X[100:140] = X[77]                                                                 # and a run of identical rows
    ids = rng.permutation(N).astype(np.int64) + 1
    idx = FlatIPIndex(d)
    idx.add_with_ids(X, ids)
    S = sel_ref.scores_f64(X, Q)
    assert len(np.unique(S)) < 80
    for sel in (IDSelectorNot(IDSelectorBatch(ids[[77, 101, 102, 3000]])), IDSelectorBatch(ids[::3]), IDSelectorRange(1, N + 1)):
        mask = sel_ref.resolve(ids, sel)
        for k in (1, 10, 100, 1000):
            D, I = idx.search(Q, k, params=SearchParameters(sel=sel))
            Do, Io, _ = sel_ref.filtered_topk(S, np.arange(N), mask, ids, k)
            assert np.array_equal(I, Io) and np.array_equal(D, Do), k                  # exact scores, exact order
    D1, I1 = idx.search(Q, 50, params=SearchParameters(sel=IDSelectorRange(1, N + 1)))
    D0, I0 = idx.search(Q, 50)
    assert np.array_equal(I1, I0) and np.array_equal(D1, D0)                           # every row selected: the plain answer


def test_flat_filtered_search_leaves_the_shadows_alone():
    N, d, k = 1 << 18, 64, 10
    X = sel_ref.unit_rows(N, d, 3)
    Q = sel_ref.unit_rows(1, d, 4)
    ids = np.arange(N, dtype=np.int64) + 1
    idx = FlatIPIndex(d, shadow=True)
    idx.add_with_ids(X, ids)
    D0, I0 = idx.search(Q, k)
    before = idx.shadow_counts()
    assert sum(before) == 1                                                            # the two-stage search answered
    sel = IDSelectorRange(1000, 5000)
    D, I = idx.search(Q, k, params=SearchParameters(sel=sel))
    assert idx.shadow_counts() == before                                               # the filtered search did not go near them
    S64 = sel_ref.scores_f64(X, Q)
    check_flat(D, I, S64, sel_ref.resolve(ids, sel), ids, k, "shadowed index")
    D1, I1 = idx.search(Q, k)
    assert np.array_equal(D1.view(np.uint32), D0.view(np.uint32)) and np.array_equal(I1, I0)
    assert sum(idx.shadow_counts()) == 2


def test_flat_refuses_bad_params_and_resolves_again_after_add():
    d = 64
    X = sel_ref.unit_rows(3000, d, 8)
    ids = np.arange(3000, dtype=np.int64) * 2
    idx = FlatIPIndex(d)
    idx.add_with_ids(X[:2000], ids[:2000])
    with pytest.raises(ValueError):
        idx.search(X[:1], 5, params={"sel": None})
    with pytest.raises(ValueError):
        idx.search(X[:1], 5, params=SearchParametersIVF(nprobe=4))
    sel = IDSelectorRange(3000, 6000)                                                  # rows 1500 .. 2999
    D, I = idx.search(X[2500:2501], 5, params=SearchParameters(sel=sel))
    assert ((I >= 3000) & (I < 4000)).all()
    first = sel.resolve(idx)
    assert sel.resolve(idx) is first and first.n == 2000                               # cached per index and row count
    other = FlatIPIndex(d)
    other.add_with_ids(X[:100], ids[:100])
    with pytest.raises(ValueError):
        other.search_device(dev(X[:1]), 5, sel=first)                                  # resolved against another row count
    idx.add_with_ids(X[2000:], ids[2000:])
    D, I = idx.search(X[2500:2501], 5, params=SearchParameters(sel=sel))
    assert I[0, 0] == 5000 and abs(D[0, 0] - 1.0) < 1e-5                               # the new rows are selectable
    assert sel.resolve(idx) is not first and sel.resolve(idx).n == 3000
    with pytest.raises(ValueError):
        idx.search_device(dev(X[:1]), 5, sel=first)                                    # the stale resolution is refused, not used


# --------------------------------------------------------------------------------------------------------------------- IVFFlat
def check_against(D, I, Do, Io, tol=TOL):
    """tests/test_gpu_ivf.py: check_against_oracle"""
    assert D.shape == Do.shape and I.dtype == np.int64
    assert np.allclose(D, Do, atol=tol)
    gap_ok = np.ones_like(Io, dtype=bool)
    gap_ok[:, 1:] &= (Do[:, :-1] - Do[:, 1:]) > tol
    gap_ok[:, :-1] &= (Do[:, :-1] - Do[:, 1:]) > tol
    assert np.array_equal(I[gap_ok], Io[gap_ok])


def ivf_filtered_oracle(Xs, ids_s, off, Q, probes, k, mask):
    """oracle/ivf_ref.ivf_search among the rows with mask[position] set: the same probes, then the mask"""
    D = np.full((Q.shape[0], k), NEG, dtype=np.float32)
    I = np.full((Q.shape[0], k), -1, dtype=np.int64)
    for q in range(Q.shape[0]):
        rows = np.concatenate([np.arange(off[l], off[l + 1]) for l in probes[q] if l >= 0] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        rows = rows[mask[rows]]
        if rows.size == 0:
            continue
        s = (Xs[rows].astype(np.float32) @ Q[q].astype(np.float32)).astype(np.float32)
        order = np.lexsort((rows, -s.astype(np.float64)))[:k]
        D[q, :len(order)] = s[order]
        I[q, :len(order)] = ids_s[rows[order]]
    return D, I


@pytest.mark.parametrize("N,d,nlist,nprobe,nq,k", [(20000, 128, 64, 8, 5, 10), (5000, 512, 37, 37, 3, 10), (30000, 64, 200, 1, 9, 5),
                                                   (3000, 768, 16, 4, 2, 100), (30000, 64, 400, 128, 6, 10)])
def test_ivfflat_filtered_search_equals_the_restatement(N, d, nlist, nprobe, nq, k):
    X = sel_ref.unit_rows(N, d, N + d)
    Q = sel_ref.unit_rows(nq, d, 7)
    idx = IVFFlatIPIndex(d, nlist)
    idx.train(X[: max(nlist * 20, min(N, 4000))])
    ids = np.random.default_rng(N).permutation(N).astype(np.int64) * 3 + 11
    for s in range(0, N, 7000):
        idx.add_with_ids(X[s:s + 7000], ids[s:s + 7000])
    idx.nprobe = nprobe
    c, Xs, ids_s, off = idx.lists_host()
    probes = idx.probes_device(dev(Q), min(nprobe, nlist)).cpu().numpy()
    rng = np.random.default_rng(N + 1)
    for sel in (IDSelectorBatch(rng.permutation(ids)[: N // 10]), IDSelectorNot(IDSelectorBatch(rng.permutation(ids)[: N // 2])),
                IDSelectorRange(11, 11 + 3 * 40), IDSelectorRange(-5, 10 ** 9), IDSelectorBatch([ids[5]]), IDSelectorBatch([1, 4])):
        mask = sel_ref.resolve(ids_s, sel)                                             # by position IN LIST ORDER
        D, I = idx.search(Q, k, params=SearchParametersIVF(sel=sel))
        Do, Io = ivf_filtered_oracle(Xs, ids_s, off, Q, probes, k, mask)
        check_against(D, I, Do, Io)
        assert np.array_equal(I == -1, Io == -1) and np.all(D[I == -1] == NEG)
        assert np.isin(I[I >= 0], ids_s[mask]).all()
    D1, I1 = idx.search(Q, k, params=SearchParametersIVF(sel=IDSelectorRange(-5, 10 ** 9)))
    D0, I0 = idx.search(Q, k)
    assert np.array_equal(D1.view(np.uint32), D0.view(np.uint32)) and np.array_equal(I1, I0)       # every row selected: the plain bits


# ----------------------------------------------------------------------------------------------------------------------- IVFPQ
def scan_case(m, nlist=48, seed=0):
    """tests/test_gpu_ivfpq.py: lists of 0 .. ~400 rows (some empty), a tenth of the rows exact copies of their list's first row"""
    rng = np.random.default_rng(seed + m)
    sizes = rng.integers(0, 400, nlist)
    sizes[[3, 17, nlist - 1]] = 0
    list_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(list_off[-1])
    codes = rng.integers(0, 256, (N, m)).astype(np.uint8)
    first = list_off[ivfpq_ref.list_of_rows(list_off)]
    dup = rng.random(N) < 0.1
    codes[dup] = codes[first[dup]]
    ids = rng.permutation(N).astype(np.int64) * 5 + 3
    return codes, list_off, ids


def gpu_pq_scan(codes_d, N, m, off_d, nlist, ids_d, lut, probes, bias, k, keep_d):
    """wise_ivfpq_scan_sel (keep_d given) or wise_ivfpq_scan through the C ABI"""
    lib = _lib.lib()
    nq, nprobe = probes.shape
    need = lib.wise_ivfpq_scan_workspace_bytes(nq, nprobe, k, m)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    l_d, p_d, b_d = dev(lut), dev(probes), dev(bias)
    D = torch.empty(nq, k, dtype=torch.float32, device="cuda")
    I = torch.empty(nq, k, dtype=torch.int64, device="cuda")
    head = (codes_d.data_ptr(), N, m, off_d.data_ptr(), nlist, _lib.ptr(ids_d), l_d.data_ptr(), nq, p_d.data_ptr(), b_d.data_ptr(), nprobe, k)
    tail = (D.data_ptr(), I.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    if keep_d is None:
        _lib.check(lib.wise_ivfpq_scan(*head, *tail), "wise_ivfpq_scan")
    else:
        _lib.check(lib.wise_ivfpq_scan_sel(*head, keep_d.data_ptr(), *tail), "wise_ivfpq_scan_sel")
    torch.cuda.synchronize()
    return D.cpu().numpy(), I.cpu().numpy()


@pytest.mark.parametrize("k", [1, 10, 100, 1000])
@pytest.mark.parametrize("m", [8, 16, 64, 128])
def test_pq_scan_sel_is_bit_equal_to_the_restatement(m, k):
    codes, list_off, ids = scan_case(m)
    nlist, N = len(list_off) - 1, codes.shape[0]
    codes_d, off_d, ids_d = dev(codes), dev(list_off), dev(ids)
    rng = np.random.default_rng(100 + m + k)
    masks = {"tenth": rng.random(N) < 0.1, "most": rng.random(N) < 0.9, "few": rng.random(N) < 0.002, "none": np.zeros(N, bool),
             "all": np.ones(N, bool)}
    for nq in (1, 3, 64):
        lut = (rng.standard_normal((nq, m, 256)) / np.sqrt(m)).astype(np.float32)
        for nprobe in (1, 8, 1024):
            probes = np.full((nq, nprobe), -1, dtype=np.int64)
            for q in range(nq):
                probes[q, :min(nprobe, nlist)] = rng.permutation(nlist)[:nprobe]
            if nprobe > 1:
                probes[rng.random(probes.shape) < 0.1] = -1                            # a probe of -1, and lists 3, 17, 47 are empty
            bias = rng.standard_normal((nq, nprobe)).astype(np.float32)
            for name, mask in masks.items():
                what = f"m={m} k={k} nq={nq} nprobe={nprobe} {name}"
                keep_d = dev(sel_ref.bitmap(mask).view(np.int32))
                for with_ids in (None, ids):                                           # None: the positions mode of the R types
                    D, I = gpu_pq_scan(codes_d, N, m, off_d, nlist, None if with_ids is None else ids_d, lut, probes, bias, k, keep_d)
                    Do, Io = sel_ref.pq_scan(codes, list_off, with_ids, lut, probes, bias, k, mask)
                    assert np.array_equal(D.view(np.uint32), Do.view(np.uint32)), what  # bit for bit
                    assert np.array_equal(I, Io), what                                  # ids included; ties: the lower position
                if name == "all":                                                      # every row selected: wise_ivfpq_scan's bits
                    Dp, Ip = gpu_pq_scan(codes_d, N, m, off_d, nlist, ids_d, lut, probes, bias, k, None)
                    assert np.array_equal(D.view(np.uint32), Dp.view(np.uint32)) and np.array_equal(I, Ip), what   # (D, I: the run with ids)
                if name == "none":
                    assert (I == -1).all() and (D == NEG).all(), what


# ---------------------------------------------------------------------------------------------------- the PQ-family index classes
def search_and_probes(idx, Q, k, params):
    """idx.search(Q, k, params) and the probes that very search took from its coarse stage (tests/test_gpu_ivfopq.py)"""
    seen, real = [], idx._coarse.probes_device
    idx._coarse.probes_device = lambda q, nprobe: seen.append(real(q, nprobe)) or seen[-1]
    try:
        D, I = idx.search(Q, k, params=params)
    finally:
        del idx._coarse.probes_device
    assert len(seen) == 1
    return D, I, seen[0].contiguous()


def gpu_tables(idx, Q_d, probes_d):
    """bias and table as the index's own search computes them (the table from the rotated queries on the OPQ types)"""
    lib, st = _lib.lib(), _lib.stream_ptr()
    nq, nprobe = probes_d.shape
    bias = torch.empty(nq, nprobe, dtype=torch.float32, device="cuda")
    _lib.check(lib.wise_pq_bias(Q_d.data_ptr(), idx.centroids.data_ptr(), probes_d.data_ptr(), nq, nprobe, idx.nlist, idx.d,
                                bias.data_ptr(), st), "wise_pq_bias")
    tq = idx._table_queries(Q_d)
    lut = torch.empty(nq, idx.m, 256, dtype=torch.float32, device="cuda")
    _lib.check(lib.wise_pq_lut(tq.data_ptr(), idx.codebooks.data_ptr(), nq, idx.d, idx.m, lut.data_ptr(), st), "wise_pq_lut")
    return bias.cpu().numpy(), lut.cpu().numpy()


def small_set():
    N, d = 20000, 64
    X = ivfpq_ref.clustered_unit_rows(N, d, 140, 0.3, 31)
    Q = sel_ref.unit_rows(16, d, 4) * 0.2 + X[100:116]
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    return X, Q, np.random.default_rng(9).permutation(N).astype(np.int64) * 3 + 11


def build_index(kind_name, X, ids, nlist=100, m=16):
    d = X.shape[1]
    idx = {"pq": lambda: IVFPQIPIndex(d, nlist, m), "r8": lambda: IVFPQRefineIPIndex(d, nlist, m, 8),
           "r16": lambda: IVFPQRefineIPIndex(d, nlist, m, 16), "opq": lambda: IVFOPQIPIndex(d, nlist, m),
           "opqr8": lambda: IVFOPQRefineIPIndex(d, nlist, m, 8), "opqr16": lambda: IVFOPQRefineIPIndex(d, nlist, m, 16),
           "flat": lambda: IVFFlatIPIndex(d, nlist)}[kind_name]()
    if kind_name.startswith("opq"):
        idx.opq_niter = 3
    idx.train(X)
    for s in range(0, X.shape[0], 7000):
        idx.add_with_ids(X[s:s + 7000], ids[s:s + 7000])
    return idx


@pytest.mark.parametrize("kind_name", ["pq", "r8", "r16", "opq", "opqr8", "opqr16"])
def test_pq_index_filtered_search_equals_the_restatement_on_its_own_state(kind_name):
    X, Q, ids = small_set()
    N, k = X.shape[0], 10
    idx = build_index(kind_name, X, ids)
    c, cb, codes, ids_s, off = idx.lists_host()
    refine = hasattr(idx, "kind")
    if refine:
        rows, scales = idx.store_host()
    rng = np.random.default_rng(17)
    Q_d = dev(Q)
    selectors = (IDSelectorBatch(rng.permutation(ids)[: N // 10]), IDSelectorNot(IDSelectorRange(11, 11 + 3 * (N // 2))),
                 IDSelectorBatch(rng.permutation(ids)[:7]), IDSelectorBatch([1, 4]))
    for nprobe, k_factor in ((8, 5), (100, 50)):
        idx.nprobe = nprobe
        if refine:
            idx.k_factor = k_factor
        for sel in selectors:
            mask = sel_ref.resolve(ids_s, sel)                                         # by position in list order
            D, I, probes_d = search_and_probes(idx, Q, k, SearchParametersIVF(sel=sel))
            bias, lut = gpu_tables(idx, Q_d, probes_d)
            probes = probes_d.cpu().numpy()
            if refine:                                                                 # the candidates are the best SELECTED rows
                kc = idx.candidates(k)
                _, cand = sel_ref.pq_scan(codes, off, None, lut, probes, bias, kc, mask)
                Do, Io = rr.refine(rows, idx.kind, scales, ids_s, Q, cand, k)
            else:
                Do, Io = sel_ref.pq_scan(codes, off, ids_s, lut, probes, bias, k, mask)
            what = (kind_name, nprobe, type(sel).__name__, int(mask.sum()))
            assert np.array_equal(D.view(np.uint32), Do.view(np.uint32)) and np.array_equal(I, Io), what      # bit for bit
            assert np.isin(I[I >= 0], ids_s[mask]).all(), what
            assert np.all(D[I == -1] == NEG)
    assert (I == -1).all()                                                             # the last selector holds no id of the index


# ------------------------------------------------------------------------------------- every index type: only selected ids, padding
@pytest.mark.parametrize("kind_name", ["flatip", "flat", "pq", "r8", "r16", "opq", "opqr8", "opqr16"])
def test_no_unselected_id_and_padding_in_the_tail(kind_name):
    N, d, k = 6000, 64, 10
    X = ivfpq_ref.clustered_unit_rows(N, d, 40, 0.3, 3)
    ids = np.random.default_rng(2).permutation(N).astype(np.int64) * 3 + 11
    if kind_name == "flatip":
        idx = FlatIPIndex(d)
        idx.add_with_ids(X, ids)
        params = SearchParameters
    else:
        idx = build_index(kind_name, X, ids, nlist=30)
        idx.nprobe = 30                                                                # every list: every selected row is met
        params = SearchParametersIVF
    Q = X[:9]
    chosen = ids[[5, 900, 901, 2000, 5999]]
    for sel, want in ((IDSelectorBatch(chosen), set(chosen.tolist())), (IDSelectorBatch(np.concatenate([chosen, [1, 4]])), set(chosen.tolist())),
                      (IDSelectorNot(IDSelectorBatch(ids[3:])), set(ids[:3].tolist())), (IDSelectorRange(0, 11), set())):
        D, I = idx.search(Q, k, params=params(sel=sel))
        n = len(want)
        assert all(set(row[:n].tolist()) == want for row in I), (kind_name, I)          # each selected row once, nothing else
        assert (I[:, n:] == -1).all() and (D[:, n:] == NEG).all() and (D[:, :n] > NEG).all()
        assert np.all(np.diff(D, axis=1) <= 0)
    D, I = idx.search(Q, k, params=params(sel=IDSelectorNot(IDSelectorBatch(ids[:9]))))   # exclude the query rows themselves
    assert (I >= 0).all() and not np.isin(I, ids[:9]).any()
    if kind_name in ("flatip", "flat"):                                                # exact scores: the plain search does return them
        assert (idx.search(Q, k)[1][:, 0] == ids[:9]).all()


# ------------------------------------------------------------------------------------------------- nprobe override, re-resolution
def test_nprobe_override_is_for_one_call_and_added_rows_become_selectable():
    X, Q, ids = small_set()
    N = X.shape[0]
    idx = build_index("flat", X[:15000], ids[:15000])
    idx.nprobe = 2
    sel = IDSelectorBatch(ids[::2])
    D2, I2, probes2 = search_and_probes(idx, Q, 10, SearchParametersIVF(sel=sel))
    D50, I50, probes50 = search_and_probes(idx, Q, 10, SearchParametersIVF(sel=sel, nprobe=50))
    assert probes2.shape == (16, 2) and probes50.shape == (16, 50)                     # the coarse stage saw the override
    assert idx.nprobe == 2                                                             # for that call only
    idx.nprobe = 50
    D50b, I50b = idx.search(Q, 10, params=SearchParametersIVF(sel=sel))
    idx.nprobe = 2
    assert np.array_equal(I50, I50b) and np.array_equal(D50, D50b)
    D, I = idx.search(Q, 10, params=SearchParametersIVF(nprobe=50))                    # no selector: the plain scan under the override
    idx.nprobe = 50
    Dp, Ip = idx.search(Q, 10)
    assert np.array_equal(I, Ip) and np.array_equal(D, Dp)
    with pytest.raises(ValueError):
        idx.search(Q, 10, params=SearchParameters)                                     # the class, not an object
    first = sel.resolve(idx)
    assert first.n == 15000 and sel.resolve(idx) is first
    idx.add_with_ids(X[15000:], ids[15000:])                                           # the cached resolution is stale now
    new = IDSelectorBatch(ids[15000:])
    idx.nprobe = 100
    D, I = idx.search(X[15000:15008], 3, params=SearchParametersIVF(sel=new))
    assert (I[:, 0] == ids[15000:15008]).all()
    D, I = idx.search(X[15000:15008:2], 3, params=SearchParametersIVF(sel=sel))        # even rows: in ids[::2]
    assert sel.resolve(idx) is not first and sel.resolve(idx).n == N
    assert (I[:, 0] == ids[15000:15008:2]).all()
    with pytest.raises(ValueError):
        idx.search_device(dev(Q), 3, sel=first)
    assert isinstance(first, ResolvedSelector)


# ------------------------------------------------------------------------------------------------------- through SearchIndexFactory
def test_search_index_factory_within(tmp_path, monkeypatch):
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    from wise_amd.index.search_index_factory import SearchIndexFactory

    fdir, idir = tmp_path / "features", tmp_path / "index"
    fdir.mkdir()
    X = ivfpq_ref.clustered_unit_rows(3000, 512, 40, 0.3, 9)
    st = FeatureStoreFactory.create_store(FeatureStoreType.WEBDATASET, "video", str(fdir))
    st.enable_write(2048, 20 * 1024 * 1024)
    for i in range(X.shape[0]):
        st.add(i + 1, X[i:i + 1])
    st.close()
    within = np.arange(100, 130, dtype=np.int64)                                       # "the vectors of one video"
    for index_type in ("IndexFlatIP", "IndexIVFPQ8"):
        si = SearchIndexFactory("video", "mlfoundations/open_clip/ViT-B-32/seeded-0", {"features_dir": fdir, "index_dir": idir})
        si.create_index(index_type)
        assert si.load_index(index_type) is True
        if hasattr(si.index, "nprobe"):
            si.index.nprobe = si.index.nlist
        dist, ids = si.search("video", "dog", topk=5, within=within)
        assert dist.shape == (5,) and ids.shape == (5,) and np.isin(ids, within).all() and len(set(ids.tolist())) == 5
        assert np.all(np.diff(dist) <= 0)
        dist, ids = si.search("video", "dog", topk=50, within=IDSelectorBatch(within))
        assert set(ids[:30].tolist()) == set(within.tolist()) and (ids[30:] == -1).all()      # 30 selected rows, then padding
        dist, ids = si.search("video", "dog", topk=5, within=IDSelectorNot(IDSelectorRange(1, 2901)))
        assert (ids > 2900).all()
        plain = si.search("video", "dog", topk=5)
        assert plain[1].shape == (5,) and (plain[1] >= 1).all()
        both = si.search_batch("video", ["dog", "a cat"], topk=5, within=within)
        assert len(both) == 2 and all(np.isin(i, within).all() for _, i in both)
        assert np.array_equal(both[0][1], si.search("video", "dog", topk=5, within=within)[1])

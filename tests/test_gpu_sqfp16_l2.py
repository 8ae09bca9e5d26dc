"""-m gpu: IndexSQfp16L2 (csrc/l2_sq16.hip, wise_amd/index/flat_sq.py: FlatSQfp16L2Index) — every path bit for bit against
tests/sqfp16_l2_ref.py, through the C ABI and through the class.

(1) the exact scan: d = 16 (C = 1, no fold, 64 rows a load), 48 (C = 3: a fold over an odd count, idle lanes), 512, 1024 (one row a
    load); N in {0, 1, 257, 5000}; nq in {1, 3, 4, 5} (the pass split 4 + 1); k in {1, 10, 2048 with N < k}; duplicate rows, rows
    with binary16 subnormals, rows of lengths 1 .. 4;
(2) the scan over positions and the selectors; (3) range count / fill; (4) wise_l2sq16_prepare and the batched search against the
    exact scan's bits, with an overflowing list and a query without a binary16 image; (5) graph capture; (6) argument checks;
(7) the class: construction, mutation, routing; (8) slices merged in rank order, and the plugin on RCCL."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import sqfp16_l2_ref as ref
from wise_amd import _lib
from wise_amd.index.sharded import merge_device, shard_range

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
WISE_E_INVALID = -1
PAD = ref.PAD
SQ_T = 4                                                                # wave-loads in flight per wave (csrc/sq_codec.h)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    if a.dtype == np.float32:
        return a.view(np.int32)
    return a.view(np.int16) if a.dtype == np.float16 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def block_rows(d):
    """rows one block of the exact scan takes before the next block's rows begin: 4 waves x SQ_T wave-loads x (64 / (d / 16)) rows"""
    return 4 * SQ_T * (64 // (d // 16))


def make_rows(N, d, seed):
    """halves [N,d] of rows of lengths 1 .. 4 with a duplicate pair on both sides of a block boundary, one at the two ends, and rows
    whose components are binary16 subnormals.  Returns (halves, rows whose copies exist)."""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((N, d)) / np.sqrt(d) * rng.uniform(1.0, 4.0, size=(N, 1))).astype(np.float32)
    for r in range(3, N, 97):
        X[r] *= np.float32(2.0 ** -16)                                  # components around 2^-18: below binary16's 2^-14
    H = ref.encode(X)
    dup = []
    B = block_rows(d)
    if N > B + 1:
        H[B] = H[B - 1]
        dup.append(B - 1)
    if N > 2:
        H[N - 1] = H[1]
        dup.append(1)
    if N > 3:
        mag = np.abs(H[3].astype(np.float32))
        assert ((mag > 0) & (mag < 2.0 ** -14)).any()                   # subnormal halves are stored
    return H, dup


def make_queries(H, dup, nq, seed):
    d = H.shape[1]
    rng = np.random.default_rng(seed)
    Q = (rng.standard_normal((nq, d)) / np.sqrt(d) * 2.0).astype(np.float32)
    for i, r in enumerate(dup[:nq]):
        Q[i] = H[r].astype(np.float32) + np.float32(1e-3) * Q[i]         # its copies share the smallest distance
    if H.shape[0] > 3 and nq > 2:
        Q[nq - 1] = H[3].astype(np.float32) * np.float32(1.5)            # beside a subnormal row
    return Q


def gpu_topk(Hd, N, d, Qd, k, ids=None, id_base=0, pos=None):
    lib = _lib.lib()
    nq = Qd.shape[0]
    D = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    I = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    n_items = N if pos is None else pos.numel()
    need = lib.wise_l2sqfp16_topk_workspace_bytes(n_items, d, nq, k)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    if pos is None:
        rc = lib.wise_l2sq16_topk(_lib.ptr(Hd), N, d, Qd.data_ptr(), nq, k, _lib.ptr(ids), id_base, D.data_ptr(), I.data_ptr(),
                                  ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    else:
        rc = lib.wise_l2sq16_topk_pos(_lib.ptr(Hd), N, d, _lib.ptr(pos), pos.numel(), Qd.data_ptr(), nq, k, _lib.ptr(ids), id_base,
                                      D.data_ptr(), I.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "wise_l2sq16_topk")
    return D, I


# ------------------------------------------------------------------------------------------------------------------ (1) exact scan
@pytest.mark.parametrize("d", [16, 48, 512, 1024])
@pytest.mark.parametrize("N", [0, 1, 257, 5000])
def test_exact_scan_bit_for_bit(d, N):
    H, dup = make_rows(N, d, 100 + d + N)
    Q = make_queries(H, dup, 5, 7)
    S = ref.dists(H, Q)                                                  # once per shape, shared by every case below
    if N:                                                                # the restatement against float64, within its rounding term
        assert (np.abs(S.astype(np.float64) - ref.real_dists(H, Q)) <= ref.rounding_term(d, Q, H)[:, None]).all()
    ids = np.random.default_rng(1).permutation(N).astype(np.int64) * 3 + 11
    Hd, Qd, idd = _dev(H).reshape(N, d), _dev(Q), _dev(ids)
    if N > block_rows(d) + 1:                                            # the duplicates: equal distances, the lower position first
        D, I = gpu_topk(Hd, N, d, Qd[:1], 10)
        I = I.cpu().numpy()[0]
        assert I[0] == block_rows(d) - 1 and I[1] == block_rows(d) and _bits(D)[0, 0] == _bits(D)[0, 1]
    for nq in (1, 3, 4, 5):
        for k in (1, 10, 2048):
            Dr, Ir = ref.topk(H, Q[:nq], k, S=S[:nq], id_base=5)
            D, I = gpu_topk(Hd, N, d, Qd[:nq], k, id_base=5)
            assert _same(D, Dr) and _same(I, Ir), (d, N, nq, k, "positions")
            Dr, Ir = ref.topk(H, Q[:nq], k, ids=ids, S=S[:nq])
            D, I = gpu_topk(Hd, N, d, Qd[:nq], k, ids=idd)
            assert _same(D, Dr) and _same(I, Ir), (d, N, nq, k, "ids")
            if N < k:                                                    # padding: faiss's for L2
                assert (Ir[:, N:] == -1).all() and (Dr[:, N:] == PAD).all() and PAD > 0
            assert (np.diff(D.cpu().numpy(), axis=1) >= 0).all()         # ascending


# ------------------------------------------------------------------------------------------------------------------ (2) positions
def test_position_scan_and_selectors():
    from wise_amd.index.flat_sq import FlatSQfp16L2Index
    from wise_amd.index.selector import IDSelectorBatch, IDSelectorNot, IDSelectorRange, SearchParameters

    d, N = 48, 5000
    H, dup = make_rows(N, d, 31)
    Q = make_queries(H, dup, 5, 9)
    S = ref.dists(H, Q)
    ids = np.arange(N, dtype=np.int64) * 2 + 1
    Hd, Qd, idd = _dev(H), _dev(Q), _dev(ids)
    rng = np.random.default_rng(2)
    sets = {"empty": np.zeros(0, np.int64), "one": np.array([block_rows(d)], np.int64), "every": np.arange(N, dtype=np.int64),
            "sparse": np.sort(rng.permutation(N)[:137]).astype(np.int64),
            "dups": np.array([1, block_rows(d) - 1, block_rows(d), N - 1], np.int64)}
    for name, pos in sets.items():
        pd = _dev(pos) if pos.size else torch.zeros(0, dtype=torch.int64, device="cuda")
        for nq, k in ((1, 1), (5, 10), (5, 100)):
            Dr, Ir = ref.topk_pos(H, Q[:nq], k, pos, ids=ids, S=S[:nq])
            D, I = gpu_topk(Hd, N, d, Qd[:nq], k, ids=idd, pos=pd)
            assert _same(D, Dr) and _same(I, Ir), (name, nq, k)
        Dr, Ir = ref.topk_pos(H, Q[:2], 10, pos, S=S[:2], id_base=3)
        D, I = gpu_topk(Hd, N, d, Qd[:2], 10, id_base=3, pos=pd)
        assert _same(D, Dr) and _same(I, Ir), name
    # through the class: an empty selection, one row, Not, Batch, Range
    idx = FlatSQfp16L2Index(d).adopt(Hd, idd)
    chosen = np.sort(rng.permutation(ids)[:300])
    sels = {"empty": (IDSelectorBatch(np.array([0], np.int64)), np.zeros(N, bool)),          # id 0 is no row's
            "one": (IDSelectorBatch(ids[77:78]), np.arange(N) == 77),
            "not": (IDSelectorNot(IDSelectorRange(100, 9000)), ~((ids >= 100) & (ids < 9000))),
            "batch": (IDSelectorBatch(chosen), np.isin(ids, chosen)),
            "range": (IDSelectorRange(1500, 2500), (ids >= 1500) & (ids < 2500))}
    for name, (sel, mask) in sels.items():
        D, I = idx.search(Q, 20, params=SearchParameters(sel=sel))
        Dr, Ir = ref.topk_pos(H, Q, 20, np.flatnonzero(mask), ids=ids, S=S)
        assert _same(D, Dr) and _same(I, Ir), name
        if name == "empty":
            assert (I == -1).all() and (D == PAD).all()


# ------------------------------------------------------------------------------------------------------------------ (3) range
@pytest.mark.parametrize("d", [16, 512])
def test_range_search_is_the_prefix_of_the_exact_scan(d):
    from wise_amd.index.flat_sq import FlatSQfp16L2Index
    from wise_amd.index.selector import IDSelectorBatch

    N, nq = 5000, 5
    H, dup = make_rows(N, d, 41 + d)
    Q = make_queries(H, dup, nq, 10)
    S = ref.dists(H, Q)
    ids = np.random.default_rng(3).permutation(N).astype(np.int64) + 100
    idx = FlatSQfp16L2Index(d).adopt(_dev(H), _dev(ids))
    D2k, I2k = gpu_topk(idx._H, N, d, _dev(Q), 2048, ids=idx._ids)
    D2k, I2k = D2k.cpu().numpy(), I2k.cpu().numpy()
    chosen = np.sort(np.random.default_rng(4).permutation(ids)[:N // 3])
    keep = np.isin(ids, chosen)
    kth = np.sort(S, axis=1)
    # a few, many, none (a radius EQUAL to the smallest distance: strictly below it there is nothing), equal to one row's distance in
    # the middle (that row is no hit), every row
    for radius in (float(kth[:, 40].min()), float(kth[:, 1500].max()), float(S.min()), float(kth[2, 100]), 3.0e38):
        for sel, mask in ((None, None), (IDSelectorBatch(chosen), keep)):
            lims, D, I = (t.cpu().numpy() for t in idx.range_search_device(_dev(Q), radius, sel=sel, chunk=2))
            lr, Dr, Ir = ref.range_search(H, Q, radius, ids=ids, keep=mask, S=S)
            assert np.array_equal(lims, lr) and _same(D, Dr) and _same(I, Ir), (d, radius, sel is not None)
            if mask is None:                                             # a prefix of the exact scan's top-2048 under dist < radius
                for q in range(nq):
                    n = min(int(lims[q + 1] - lims[q]), 2048)
                    assert n == min(int((S[q] < np.float32(radius)).sum()), 2048)
                    assert _same(D[lims[q]:lims[q] + n], D2k[q, :n]) and _same(I[lims[q]:lims[q] + n], I2k[q, :n])
    lims, D, I = idx.range_search(Q[2:3], float(kth[2, 100]))            # strict: the row AT the radius is left out
    assert lims.tolist() == [0, int((S[2] < kth[2, 100]).sum())] and (D < kth[2, 100]).all()
    lims, D, I = idx.range_search(Q, float(S.min()))
    assert lims.tolist() == [0] * (nq + 1) and D.size == 0 and I.size == 0
    lims, D, _ = idx.range_search(Q[:1], 3.0e38)
    assert lims.tolist() == [0, N] and (np.diff(D) >= 0).all()
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            idx.range_search(Q, bad)


# ------------------------------------------------------------------------------------------------------------------ (4) batched
def gpu_prepare(Hd, N, d):
    half = torch.full((max(N, 1),), -1.0, dtype=torch.float32, device="cuda")
    norms = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().wise_l2sq16_prepare(_lib.ptr(Hd) if N else 0, N, d, half.data_ptr(), norms.data_ptr(), _lib.stream_ptr()),
               "wise_l2sq16_prepare")
    return half[:N], norms


def gpu_batched(Hd, prep, N, d, Qd, k, ids=None, id_base=0, counters=None):
    lib = _lib.lib()
    half, norms = prep
    nq = Qd.shape[0]
    D = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    I = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    need = lib.wise_l2sqfp16_topk_batched_workspace_bytes(N, d, nq, k)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _lib.check(lib.wise_l2sq16_topk_batched(Hd.data_ptr(), half.data_ptr(), norms.data_ptr(), N, d, Qd.data_ptr(), nq, k, _lib.ptr(ids),
                                            id_base, D.data_ptr(), I.data_ptr(), _lib.ptr(counters), ws.data_ptr(), ws.numel(),
                                            _lib.stream_ptr()), "wise_l2sq16_topk_batched")
    return D, I


def clustered_halves(N, d, seed, nq=130):
    """binary16 rows around 64 centres times lengths log-uniform over [1, 4] (near neighbours: many distances close to a query's
    k-th; NOT normalised) and fp32 queries beside rows, on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    c = torch.randn(64, d, device="cuda", generator=g)
    c /= c.norm(dim=1, keepdim=True)
    e = torch.randn(N, d, device="cuda", generator=g)
    X = c[torch.randint(0, 64, (N,), device="cuda", generator=g)] + 0.35 * e / e.norm(dim=1, keepdim=True)
    X = X / X.norm(dim=1, keepdim=True) * torch.exp(torch.rand(N, 1, device="cuda", generator=g) * float(np.log(4.0)))
    H = X.half().contiguous()
    Q = H[:nq].float() * (1.0 + 0.05 * torch.randn(nq, d, device="cuda", generator=g))
    return H, Q.float().contiguous()


@pytest.mark.parametrize("d", [16, 256, 1024])
@pytest.mark.parametrize("N", [0, 1, 4096])
def test_prepare_writes_the_half_norms_and_the_largest_norm(d, N):
    H, _ = make_rows(N, d, 200 + d)
    half, norms = gpu_prepare(_dev(H).reshape(N, d), N, d)
    want = ref.half_norms(H) if N else np.zeros(0, np.float32)
    assert _same(half, want) and _same(norms, np.array([ref.max_norm(want)], np.float32))
    if N:
        real = 0.5 * (H.astype(np.float64) ** 2).sum(axis=1)
        assert (np.abs(want.astype(np.float64) - real) <= d * 2.0 ** -24 * real + 1e-45).all()
        assert abs(float(norms[0]) - float(np.sqrt(2 * real.max()))) <= 1e-5 * float(np.sqrt(2 * real.max()))
    else:
        assert float(norms[0]) == 0.0


@pytest.mark.parametrize("d", [256, 1024])
@pytest.mark.parametrize("N", [4096, 20000])
def test_batched_search_has_the_bits_of_the_exact_scan(d, N):
    H, Q = clustered_halves(N, d, 50 + d)
    H[N - 95] = H[17]                                                    # equal rows far apart
    prep = gpu_prepare(H, N, d)
    assert all(_same(a, b) for a, b in zip(prep, gpu_prepare(H, N, d)))  # deterministic
    ids = _dev(np.random.default_rng(6).permutation(N).astype(np.int64) + 9)
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    asked = 0
    for nq in (3, 130):                                                  # the fewest; two passes at d <= 512 (128 + 2), three at 1024
        for k in (1, 128):
            De, Ie = gpu_topk(H, N, d, Q[:nq], k, ids=ids)
            D, I = gpu_batched(H, prep, N, d, Q[:nq], k, ids=ids, counters=counters)
            assert _same(D, De) and _same(I, Ie), (d, N, nq, k)
            asked += nq
    De, Ie = gpu_topk(H, N, d, Q[:7], 100, id_base=4)
    D, I = gpu_batched(H, prep, N, d, Q[:7], 100, id_base=4)             # no ids, no counters
    assert _same(D, De) and _same(I, Ie)
    assert int(counters.sum()) == asked
    if N == 4096:                                                        # and the exact scan is the restatement's on this data too
        Hh, Qh = H.cpu().numpy(), Q[:3].cpu().numpy()
        Dr, Ir = ref.topk(Hh, Qh, 10)
        D, I = gpu_batched(H, prep, N, d, Q[:3], 10)
        assert _same(D, Dr) and _same(I, Ir)
    else:
        # on plain clustered data every query is answered from its list: no silent fallback hides a broken collect
        assert counters.cpu().numpy().tolist() == [asked, 0]


def test_batched_overflow_is_redone_by_the_exact_scan():
    N, d, k = 20000, 256, 10
    H, Q = clustered_halves(N, d, 91)
    q = torch.randn(d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(92))
    Q[3] = 2.0 * q / q.norm()                                            # a direction of its own: no other query sees its copies
    copies = 5000                                                        # identical rows, more than a candidate list holds (4096)
    where = torch.arange(copies, device="cuda") * 3 + 5                  # spread over the whole index
    H[where] = (Q[3] * 1.01).half().repeat(copies, 1)
    prep = gpu_prepare(H, N, d)
    nq = 5
    De, Ie = gpu_topk(H, N, d, Q[:nq], k)
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    D, I = gpu_batched(H, prep, N, d, Q[:nq], k, counters=counters)
    assert _same(D, De) and _same(I, Ie)
    assert counters.cpu().numpy().tolist() == [0, nq]                    # the gated exact scan answered that pass's queries
    assert Ie[3].tolist() == where[:k].tolist() and len(set(_bits(De)[3].tolist())) == 1      # equal distances: the lowest positions
    counters.zero_()                                                     # a pass without that query is answered from the lists
    D, I = gpu_batched(H, prep, N, d, Q[:3], k, counters=counters)
    assert _same(D, De[:3]) and _same(I, Ie[:3]) and counters.cpu().numpy().tolist() == [3, 0]


def test_batched_query_without_a_binary16_image_goes_to_the_exact_scan():
    N, d, k = 4096, 256, 10
    H, Q = clustered_halves(N, d, 93, nq=6)
    Q[2, 5] = 1.0e6                                                      # beyond 65504: the image is +inf
    prep = gpu_prepare(H, N, d)
    De, Ie = gpu_topk(H, N, d, Q, k)
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    D, I = gpu_batched(H, prep, N, d, Q, k, counters=counters)
    assert _same(D, De) and _same(I, Ie) and counters.cpu().numpy().tolist() == [0, 6]
    Dr, Ir = ref.topk(H.cpu().numpy(), Q[2:3].cpu().numpy(), k)
    assert _same(D[2:3], Dr) and _same(I[2:3], Ir) and bool(torch.isfinite(D).all())


# ------------------------------------------------------------------------------------------------------------------ (5) graph capture
def test_graph_capture_of_a_search_and_of_a_range_count():
    lib = _lib.lib()
    N, d, nq, k = 8192, 256, 6, 10
    H, Q = clustered_halves(N, d, 17, nq=nq)
    half, norms = prep = gpu_prepare(H, N, d)
    De, Ie = gpu_topk(H, N, d, Q, k)
    Dw, Iw = gpu_batched(H, prep, N, d, Q, k)                            # both paths have run once before the capture
    assert _same(Dw, De) and _same(Iw, Ie)
    radius = float(De[:, 5].max())
    want_counts = (ref.dists(H.cpu().numpy(), Q.cpu().numpy()) < np.float32(radius)).sum(axis=1)
    outs = [(torch.zeros(nq, k, dtype=torch.float32, device="cuda"), torch.zeros(nq, k, dtype=torch.int64, device="cuda")) for _ in range(2)]
    wse = torch.empty(lib.wise_l2sqfp16_topk_workspace_bytes(N, d, nq, k), dtype=torch.uint8, device="cuda")
    wsb = torch.empty(lib.wise_l2sqfp16_topk_batched_workspace_bytes(N, d, nq, k), dtype=torch.uint8, device="cuda")
    wsr = torch.empty(lib.wise_l2sqfp16_range_workspace_bytes(N, d, nq), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(nq, dtype=torch.int64, device="cuda")
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = _lib.stream_ptr()
        _lib.check(lib.wise_l2sq16_topk(H.data_ptr(), N, d, Q.data_ptr(), nq, k, 0, 0, outs[0][0].data_ptr(), outs[0][1].data_ptr(),
                                        wse.data_ptr(), wse.numel(), st))
        _lib.check(lib.wise_l2sq16_topk_batched(H.data_ptr(), half.data_ptr(), norms.data_ptr(), N, d, Q.data_ptr(), nq, k, 0, 0,
                                                outs[1][0].data_ptr(), outs[1][1].data_ptr(), counters.data_ptr(), wsb.data_ptr(),
                                                wsb.numel(), st))
        _lib.check(lib.wise_l2sq16_range_count(H.data_ptr(), N, d, Q.data_ptr(), nq, radius, 0, counts.data_ptr(), wsr.data_ptr(),
                                               wsr.numel(), st))
    for rep in range(2):
        for D, I in outs:
            D.zero_()
            I.zero_()
        counts.zero_()
        g.replay()
        torch.cuda.synchronize()
        for D, I in outs:
            assert _same(D, De) and _same(I, Ie), rep
        assert counts.cpu().numpy().tolist() == want_counts.tolist()
    assert int(counters.sum()) == 2 * nq


# ------------------------------------------------------------------------------------------------------------------ (6) argument checks
def test_refusals_leave_the_outputs_untouched():
    lib = _lib.lib()
    N, d, nq, k = 4096, 256, 4, 10
    H, Q = clustered_halves(N, d, 13, nq=nq)
    half, norms = gpu_prepare(H, N, d)
    for shape in ((N, 20, nq, k), (N, 128, nq, k), (N, 320, nq, k), (N, d, 2, k), (N, d, nq, 129), (N - 1, d, nq, k), (1 << 31, d, nq, k)):
        assert lib.wise_l2sqfp16_topk_batched_workspace_bytes(*shape) == 0, shape
    need = lib.wise_l2sqfp16_topk_batched_workspace_bytes(N, d, nq, k)
    ws = torch.empty(need + 64, dtype=torch.uint8, device="cuda")
    wse = torch.empty(lib.wise_l2sqfp16_topk_workspace_bytes(N, d, nq, k), dtype=torch.uint8, device="cuda")
    wsr = torch.empty(lib.wise_l2sqfp16_range_workspace_bytes(N, d, nq), dtype=torch.uint8, device="cuda")
    D = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    I = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    counts = torch.full((nq,), 7, dtype=torch.int64, device="cuda")
    st = _lib.stream_ptr()

    def batched(rows=H.data_ptr(), hp=half.data_ptr(), np_=norms.data_ptr(), dd=d, qp=Q.data_ptr(), wsp=ws.data_ptr(), wsn=need, n=N,
                nqq=nq, kk=k):
        return lib.wise_l2sq16_topk_batched(rows, hp, np_, n, dd, qp, nqq, kk, 0, 0, D.data_ptr(), I.data_ptr(), 0, wsp, wsn, st)

    def exact(rows=H.data_ptr(), dd=d, qp=Q.data_ptr(), wsp=wse.data_ptr(), wsn=wse.numel(), n=N, nqq=nq, kk=k):
        return lib.wise_l2sq16_topk(rows, n, dd, qp, nqq, kk, 0, 0, D.data_ptr(), I.data_ptr(), wsp, wsn, st)

    def count(radius=1.0, wsn=wsr.numel(), dd=d):
        return lib.wise_l2sq16_range_count(H.data_ptr(), N, dd, Q.data_ptr(), nq, radius, 0, counts.data_ptr(), wsr.data_ptr(), wsn, st)

    bad = {"short workspace": batched(wsn=need - 1), "no workspace": batched(wsp=0), "misaligned rows": batched(rows=H.data_ptr() + 2),
           "no half-norms": batched(hp=0), "no norms": batched(np_=0), "misaligned queries": batched(qp=Q.data_ptr() + 4),
           "d = 20": batched(dd=20), "d = 128": batched(dd=128), "nq = 2": batched(nqq=2), "k = 129": batched(kk=129),
           "N = 4095": batched(n=N - 1),
           "exact short workspace": exact(wsn=wse.numel() - 512), "exact no workspace": exact(wsp=0),
           "exact misaligned rows": exact(rows=H.data_ptr() + 2), "exact d = 20": exact(dd=20), "exact d = 1040": exact(dd=1040),
           "exact nq = 0": exact(nqq=0), "exact k = 2049": exact(kk=2049), "exact N < 0": exact(n=-1),
           "range nan": count(radius=float("nan")), "range inf": count(radius=float("inf")), "range short workspace": count(wsn=8),
           "range d = 20": count(dd=20)}
    pos = torch.arange(10, dtype=torch.int64, device="cuda")
    bad["n_pos > N"] = lib.wise_l2sq16_topk_pos(H.data_ptr(), 5, d, pos.data_ptr(), 10, Q.data_ptr(), nq, k, 0, 0, D.data_ptr(), I.data_ptr(),
                                                wse.data_ptr(), wse.numel(), st)
    bad["prepare d = 20"] = lib.wise_l2sq16_prepare(H.data_ptr(), N, 20, half.data_ptr(), norms.data_ptr(), st)
    bad["prepare no half"] = lib.wise_l2sq16_prepare(H.data_ptr(), N, d, 0, norms.data_ptr(), st)
    torch.cuda.synchronize()
    assert all(rc == WISE_E_INVALID for rc in bad.values()), bad
    assert lib.wise_last_error()
    assert bool((D == 7.0).all()) and bool((I == 7).all()) and bool((counts == 7).all())
    assert batched() == 0                                                # and the good call goes through
    torch.cuda.synchronize()
    De, Ie = gpu_topk(H, N, d, Q, k)
    assert _same(D, De) and _same(I, Ie)


# ------------------------------------------------------------------------------------------------------------------ (7) the class
def test_index_class_add_adopt_remove_reconstruct():
    from wise_amd.index.flat_common import FlatIndexBase
    from wise_amd.index.flat_sq import FlatSQfp16L2Index
    from wise_amd.index.selector import IDSelectorRange

    N, d = 5000, 48
    rng = np.random.default_rng(23)
    H, _ = make_rows(N, d, 24)
    X = H.astype(np.float32) * np.float32(1.0 + 2.0 ** -13)              # fp32 rows that round to exactly these halves
    assert _same(ref.encode(X), H) and not np.array_equal(X, H.astype(np.float32))
    ids = rng.permutation(N).astype(np.int64) + 1000
    assert issubclass(FlatSQfp16L2Index, FlatIndexBase) and FlatSQfp16L2Index.metric == "l2"
    one = FlatSQfp16L2Index(d)
    one.add_with_ids(X, ids)                                             # encoded on the GPU
    chunked = FlatSQfp16L2Index(d)
    chunked.ENCODE_BYTES = 4 * d * 700                                   # several encoder chunks inside one add
    for s in range(0, N, 1234):
        chunked.add_with_ids(X[s:s + 1234], ids[s:s + 1234])
    reserved = FlatSQfp16L2Index(d)
    reserved.reserve(N)
    for s in range(0, N, 2000):
        reserved.add_halves_with_ids(H[s:s + 2000], ids[s:s + 2000])     # an index file's rows: as they are
    adopted = FlatSQfp16L2Index(d).adopt(_dev(H), _dev(ids))
    Q = make_queries(H, [1], 5, 25)
    Dr, Ir = ref.topk(H, Q, 20, ids=ids)
    for idx in (one, chunked, reserved, adopted):
        Hh, ih = idx.rows_host()
        assert Hh.dtype == np.float16 and _same(Hh, H) and np.array_equal(ih, ids)
        assert idx.ntotal == N and idx.is_trained and idx.metric == "l2" and idx.hbm_bytes() == N * (2 * d + 8)
        D, I = idx.search(Q, 20)
        assert _same(D, Dr) and _same(I, Ir)
    assert FlatSQfp16L2Index(d).adopt(_dev(H)).hbm_bytes() == N * 2 * d  # implicit ids
    want = np.array([ids[7], ids[0], 5, ids[N - 1]], dtype=np.int64)     # reconstruct_batch: the widened halves, NaN for an absent id
    rec = one.reconstruct_batch(want)
    assert np.isnan(rec[2]).all() and _same(rec[[0, 1, 3]], H[[7, 0, N - 1]].astype(np.float32))
    # remove_ids: byte for byte the index that received only the kept rows
    gone = np.sort(rng.permutation(N)[:777])
    keep = np.setdiff1d(np.arange(N), gone)
    assert reserved.remove_ids(ids[gone]) == 777 and reserved.remove_ids(ids[gone]) == 0
    fresh = FlatSQfp16L2Index(d)
    fresh.add_with_ids(X[keep], ids[keep])
    Hr, ir = reserved.rows_host()
    Hf, if_ = fresh.rows_host()
    assert Hr.tobytes() == Hf.tobytes() == H[keep].tobytes() and np.array_equal(ir, if_) and reserved.ntotal == N - 777
    D1, I1 = reserved.search(Q, 20)
    D2, I2 = fresh.search(Q, 20)
    D3, I3 = ref.topk(H[keep], Q, 20, ids=ids[keep])
    assert _same(D1, D2) and _same(I1, I2) and _same(D1, D3) and _same(I1, I3)
    reserved.add_halves_with_ids(H[gone[:50]], ids[gone[:50]])           # the reserved tensor is filled from the new end
    assert reserved.ntotal == N - 727 and reserved.rows_host()[0].tobytes() == np.concatenate([H[keep], H[gone[:50]]]).tobytes()
    assert one.remove_ids(IDSelectorRange(0, 10 ** 9)) == N and one.ntotal == 0
    D, I = one.search(Q, 3)
    assert (I == -1).all() and (D == PAD).all()
    with pytest.raises(ValueError, match="IndexSQfp16L2.*multiple of 16"):
        FlatSQfp16L2Index(40)


def test_index_class_routes_batches_to_the_matrix_cores_and_rebuilds_after_a_removal():
    from wise_amd.index.flat_sq import FlatSQfp16IPIndex, FlatSQfp16L2Index

    N, d = 1 << 18, 256
    H, Q = clustered_halves(N, d, 29, nq=40)
    ids = _dev(np.arange(N, dtype=np.int64) * 2)
    idx = FlatSQfp16L2Index(d).adopt(H, ids)
    assert FlatSQfp16L2Index.BATCH_MIN_ROWS == FlatSQfp16IPIndex.BATCH_MIN_ROWS == 1 << 18
    assert FlatSQfp16L2Index.BATCH_MIN_QUERIES >= 3
    nb = FlatSQfp16L2Index.BATCH_MIN_QUERIES
    De, Ie = gpu_topk(H, N, d, Q, 10, ids=ids)                           # the exact scan through the C ABI
    D7, I7 = idx.search_device(Q[:nb - 1], 10)                           # under the query floor: the exact scan, nothing built
    assert idx.batched_counts() == (0, 0) and idx._half is None and _same(D7, De[:nb - 1]) and _same(I7, Ie[:nb - 1])
    D8, I8 = idx.search_device(Q[:nb], 10)                               # N = 2^18 rows, the floor's batch: the matrix-core passes
    assert idx.batched_counts() == (nb, 0) and _same(D8, De[:nb]) and _same(I8, Ie[:nb])
    assert idx._half.shape == (N,) and idx._norms.shape == (1,) and idx.hbm_bytes() == N * (2 * d + 8)
    D, I = idx.search_device(Q, 10)
    assert idx.batched_counts() == (nb + 40, 0) and _same(D, De) and _same(I, Ie)
    D3, I3 = idx.search_device(Q, 200)                                   # k > 128: the exact scan
    assert sum(idx.batched_counts()) == nb + 40 and _same(I3[:, :10], Ie)
    # the half-norms go with the rows: a removal drops them, the next batch rebuilds them over the kept rows — the fresh index's bits
    gone = torch.arange(0, N, 5, device="cuda")
    keep = torch.ones(N, dtype=torch.bool, device="cuda")
    keep[gone] = False
    gone_ids = ids[gone].cpu().numpy()
    fresh = FlatSQfp16L2Index(d).adopt(H[keep].contiguous(), ids[keep].contiguous())    # (before the removal compacts H, adopted as it is)
    assert idx.remove_ids(gone_ids) == gone.numel()
    assert idx._half is None and idx._norms is None
    assert idx.rows_host()[0].tobytes() == fresh.rows_host()[0].tobytes() and np.array_equal(idx.rows_host()[1], fresh.rows_host()[1])
    idx.BATCH_MIN_ROWS = fresh.BATCH_MIN_ROWS = 4096                     # fewer than 2^18 rows are left
    Dn, In = idx.search_device(Q, 10)
    Df, If = fresh.search_device(Q, 10)
    n2 = N - gone.numel()
    assert idx._half.shape == (n2,) and _same(idx._half, fresh._half) and _same(idx._norms, fresh._norms)
    Dx, Ix = gpu_topk(fresh._H, n2, d, Q, 10, ids=fresh._ids)
    assert _same(Dn, Df) and _same(In, If) and _same(Dn, Dx) and _same(In, Ix)


# ------------------------------------------------------------------------------------------------------------------ (8) sharding
@pytest.mark.parametrize("W", [1, 3, 8])
def test_slices_merged_in_rank_order_are_the_whole_index(W):
    from wise_amd.index.flat_sq import FlatSQfp16L2Index

    N, d, nq = 5001, 48, 4
    H, dup = make_rows(N, d, 61)
    for r in range(1, W):                                                # equal rows on both sides of every slice boundary
        lo = shard_range(N, r, W)[0]
        H[lo] = H[lo - 1]
        dup.append(lo - 1)
    Q = make_queries(H, dup[-3:], nq, 12)
    ids = np.random.default_rng(7).permutation(N).astype(np.int64) + 1
    whole = FlatSQfp16L2Index(d).adopt(_dev(H), _dev(ids))
    S = ref.dists(H, Q)
    for k in (1, 10, 100):
        De, Ie = whole.search_device(_dev(Q), k)
        Dr, Ir = ref.topk(H, Q, k, ids=ids, S=S)
        assert _same(De, Dr) and _same(Ie, Ir)
        Ds, Is = [], []
        for r in range(W):
            lo, hi = shard_range(N, r, W)
            part = FlatSQfp16L2Index(d).adopt(_dev(H[lo:hi]), _dev(ids[lo:hi]))
            D, I = part.search_device(_dev(Q), k)
            Ds.append(-D)                                                # what the wrapper exchanges: the negated distances
            Is.append(I)
        D, I = merge_device(torch.stack(Ds), torch.stack(Is), k)         # wise_topk_merge
        assert _same(-D, De) and _same(I, Ie), (W, k)


def test_sharded_plugin_over_rccl_world1(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(ROOT / "tests" / "sharded_sqfp16_l2_nccl_worker.py"),
                        str(tmp_path)], env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert res["ok"], json.dumps(res)
    assert res["exchange_bytes"] == 16 * 3 * 10                          # one exchange of (score, id) planes: nq = 3, k = 10

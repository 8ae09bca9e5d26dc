"""-m gpu: IndexFlatL2 (csrc/l2_topk.hip, wise_amd/index/flat_l2.py) — every path bit for bit against tests/l2_flat_ref.py.

(1) the exact scan over shapes that take every path of it (rows per wave-load 64 .. 1, 1 / 2 / 4 queries a pass, list lengths,
    several blocks and a ragged tail), with duplicate rows across a block boundary and padding when N < k;
(2) the scan over a list of positions; (3) range count / fill through range_search.run; (4) the batched search against
    wise_l2_topk_f32 on the same data — plain clustered rows (answered from the lists), rows of norms 1e-3 .. 1e3, queries midway
    between bf16 grid points, a constructed overflow — and the refusals; (5) graph capture; (6) the index class; (7) slices merged
    in rank order, and the plugin on RCCL."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import l2_flat_ref as ref
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
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def block_rows(d):
    """rows one block of the exact scan takes before the next block's rows begin: 4 waves x SQ_T wave-loads x (64 / (d / 16)) rows"""
    return 4 * SQ_T * (64 // (d // 16))


def make_rows(N, d, seed):
    """rows [N,d] float32 of mixed lengths with a duplicate pair on both sides of a block boundary and one at the two ends.
    Returns (rows, rows whose copies exist)."""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((N, d)) / np.sqrt(d) * rng.uniform(0.5, 2.0, size=(N, 1))).astype(np.float32)
    dup = []
    B = block_rows(d)
    if N > B + 1:
        X[B] = X[B - 1]
        dup.append(B - 1)
    if N > 2:
        X[N - 1] = X[1]
        dup.append(1)
    return X, dup


def make_queries(X, dup, nq, seed):
    d = X.shape[1]
    rng = np.random.default_rng(seed)
    Q = (rng.standard_normal((nq, d)) / np.sqrt(d)).astype(np.float32)
    for i, r in enumerate(dup[:nq]):
        Q[i] = X[r] + np.float32(1e-3) * Q[i]                            # its copies share the smallest distance
    return Q


def gpu_topk(Xd, N, d, Qd, k, ids=None, id_base=0, pos=None):
    lib = _lib.lib()
    nq = Qd.shape[0]
    D = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    I = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    n_items = N if pos is None else pos.numel()
    need = lib.wise_l2_topk_workspace_bytes(n_items, d, nq, k)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    if pos is None:
        rc = lib.wise_l2_topk_f32(_lib.ptr(Xd), N, d, Qd.data_ptr(), nq, k, _lib.ptr(ids), id_base, D.data_ptr(), I.data_ptr(),
                                  ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    else:
        rc = lib.wise_l2_topk_pos_f32(_lib.ptr(Xd), N, d, _lib.ptr(pos), pos.numel(), Qd.data_ptr(), nq, k, _lib.ptr(ids), id_base,
                                      D.data_ptr(), I.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "wise_l2_topk_f32")
    return D, I


# ------------------------------------------------------------------------------------------------------------------ (1) exact scan
@pytest.mark.parametrize("d", [16, 48, 512, 1024])
@pytest.mark.parametrize("N", [0, 1, 63, 6000])
def test_exact_scan_bit_for_bit(d, N):
    X, dup = make_rows(N, d, 100 + d + N)
    Q = make_queries(X, dup, 5, 7)
    S = ref.dists(X, Q)                                                  # once per shape, shared by every case below
    if N:                                                                # the restatement against float64, within its rounding term
        assert (np.abs(S.astype(np.float64) - ref.real_dists(X, Q)) <= ref.rounding_term(d, Q, X)[:, None]).all()
    ids = np.random.default_rng(1).permutation(N).astype(np.int64) * 3 + 11
    Xd, Qd, idd = _dev(X).reshape(N, d), _dev(Q), _dev(ids)
    if N > block_rows(d) + 1:                                            # the duplicates: equal distances, the lower position first
        D, I = gpu_topk(Xd, N, d, Qd[:1], 10)
        I = I.cpu().numpy()[0]
        assert I[0] == block_rows(d) - 1 and I[1] == block_rows(d) and _bits(D)[0, 0] == _bits(D)[0, 1]
    for nq in (1, 3, 4, 5):
        for k in (1, 10, 2048):
            Dr, Ir = ref.topk(X, Q[:nq], k, S=S[:nq], id_base=5)
            D, I = gpu_topk(Xd, N, d, Qd[:nq], k, id_base=5)
            assert _same(D, Dr) and _same(I, Ir), (d, N, nq, k, "positions")
            Dr, Ir = ref.topk(X, Q[:nq], k, ids=ids, S=S[:nq])
            D, I = gpu_topk(Xd, N, d, Qd[:nq], k, ids=idd)
            assert _same(D, Dr) and _same(I, Ir), (d, N, nq, k, "ids")
            if N < k:                                                    # padding: faiss's for L2
                assert (Ir[:, N:] == -1).all() and (Dr[:, N:] == PAD).all() and PAD > 0
            assert (np.diff(D.cpu().numpy(), axis=1) >= 0).all()         # ascending


def test_exact_scan_several_blocks_and_a_ragged_tail():
    d, N = 16, 70001
    assert N > 4 * block_rows(d) and N % (64 // (d // 16)) != 0
    X, dup = make_rows(N, d, 5)
    Q = make_queries(X, dup, 5, 8)
    S = ref.dists(X, Q)
    Xd, Qd = _dev(X), _dev(Q)
    for nq, k in ((1, 10), (5, 100), (4, 1024), (2, 2048), (3, 1)):
        Dr, Ir = ref.topk(X, Q[:nq], k, S=S[:nq])
        D, I = gpu_topk(Xd, N, d, Qd[:nq], k)
        assert _same(D, Dr) and _same(I, Ir), (nq, k)
    I = gpu_topk(Xd, N, d, Qd[:2], 10)[1].cpu().numpy()
    assert I[0, :2].tolist() == [block_rows(d) - 1, block_rows(d)]       # across a block boundary
    assert I[1, :2].tolist() == [1, N - 1]                               # across the whole grid


# ------------------------------------------------------------------------------------------------------------------ (2) positions
@pytest.mark.parametrize("d", [48, 512])
def test_position_scan_equals_the_restatement_restricted(d):
    N = 6000
    X, dup = make_rows(N, d, 31 + d)
    Q = make_queries(X, dup, 5, 9)
    S = ref.dists(X, Q)
    ids = np.arange(N, dtype=np.int64) * 2 + 1
    Xd, Qd, idd = _dev(X), _dev(Q), _dev(ids)
    rng = np.random.default_rng(2)
    sets = {"empty": np.zeros(0, np.int64), "one": np.array([block_rows(d)], np.int64), "every": np.arange(N, dtype=np.int64),
            "sparse": np.sort(rng.permutation(N)[:137]).astype(np.int64),
            "dups": np.array([1, block_rows(d) - 1, block_rows(d), N - 1], np.int64)}
    for name, pos in sets.items():
        pd = _dev(pos) if pos.size else torch.zeros(0, dtype=torch.int64, device="cuda")
        for nq in (1, 5):
            for k in (1, 10, 100):
                Dr, Ir = ref.topk_pos(X, Q[:nq], k, pos, ids=ids, S=S[:nq])
                D, I = gpu_topk(Xd, N, d, Qd[:nq], k, ids=idd, pos=pd)
                assert _same(D, Dr) and _same(I, Ir), (name, nq, k)
                if name == "every":
                    Da, Ia = gpu_topk(Xd, N, d, Qd[:nq], k, ids=idd)
                    assert _same(D, Da) and _same(I, Ia)
        Dr, Ir = ref.topk_pos(X, Q[:2], 10, pos, S=S[:2], id_base=3)
        D, I = gpu_topk(Xd, N, d, Qd[:2], 10, id_base=3, pos=pd)
        assert _same(D, Dr) and _same(I, Ir), name


# ------------------------------------------------------------------------------------------------------------------ (3) range
@pytest.mark.parametrize("d", [16, 512])
def test_range_search_is_the_prefix_of_the_exact_scan(d):
    from wise_amd.index.flat_l2 import FlatL2Index
    from wise_amd.index.selector import IDSelectorBatch

    N, nq = 6000, 5
    X, dup = make_rows(N, d, 41 + d)
    Q = make_queries(X, dup, nq, 10)
    S = ref.dists(X, Q)
    ids = np.random.default_rng(3).permutation(N).astype(np.int64) + 100
    idx = FlatL2Index(d).adopt(_dev(X), _dev(ids))
    D2k, I2k = gpu_topk(idx._X, N, d, _dev(Q), 2048, ids=idx._ids)
    D2k, I2k = D2k.cpu().numpy(), I2k.cpu().numpy()
    chosen = np.sort(np.random.default_rng(4).permutation(ids)[:N // 3])
    keep = np.isin(ids, chosen)
    kth = np.sort(S, axis=1)
    # a few, many, none (strictly below the smallest distance: that distance itself is no hit), every row
    for radius in (float(kth[:, 40].min()), float(kth[:, 1500].max()), float(S.min()), 3.0e38):
        for sel, mask in ((None, None), (IDSelectorBatch(chosen), keep)):
            lims, D, I = (t.cpu().numpy() for t in idx.range_search_device(_dev(Q), radius, sel=sel, chunk=2))
            lr, Dr, Ir = ref.range_search(X, Q, radius, ids=ids, keep=mask, S=S)
            assert np.array_equal(lims, lr) and _same(D, Dr) and _same(I, Ir), (d, radius, sel is not None)
            if mask is None:                                             # a prefix of the exact scan's top-2048 under dist < radius
                for q in range(nq):
                    n = min(int(lims[q + 1] - lims[q]), 2048)
                    assert n == min(int((S[q] < np.float32(radius)).sum()), 2048)
                    assert _same(D[lims[q]:lims[q] + n], D2k[q, :n]) and _same(I[lims[q]:lims[q] + n], I2k[q, :n])
    lims, D, I = idx.range_search(Q, float(S.min()))
    assert lims.tolist() == [0] * (nq + 1) and D.size == 0 and I.size == 0
    lims, D, _ = idx.range_search(Q[:1], 3.0e38)
    assert lims.tolist() == [0, N] and (np.diff(D) >= 0).all()
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            idx.range_search(Q, bad)


# ------------------------------------------------------------------------------------------------------------------ (4) batched
def gpu_prepare(Xd, N, d):
    Xb = torch.full((N, d), 0x7fc0, dtype=torch.int16, device="cuda")
    half = torch.full((N,), -1.0, dtype=torch.float32, device="cuda")
    norms = torch.full((2,), -1.0, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().wise_l2_prepare(Xd.data_ptr(), N, d, Xb.data_ptr(), half.data_ptr(), norms.data_ptr(), _lib.stream_ptr()),
               "wise_l2_prepare")
    return Xb, half, norms


def gpu_batched(Xd, prep, N, d, Qd, k, ids=None, id_base=0, counters=None):
    lib = _lib.lib()
    Xb, half, norms = prep
    nq = Qd.shape[0]
    D = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    I = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    need = lib.wise_l2_topk_batched_workspace_bytes(N, d, nq, k)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _lib.check(lib.wise_l2_topk_batched(Xd.data_ptr(), Xb.data_ptr(), half.data_ptr(), norms.data_ptr(), N, d, Qd.data_ptr(), nq, k,
                                        _lib.ptr(ids), id_base, D.data_ptr(), I.data_ptr(), _lib.ptr(counters), ws.data_ptr(), ws.numel(),
                                        _lib.stream_ptr()), "wise_l2_topk_batched")
    return D, I


def clustered_rows(N, d, seed, nq=130):
    """unit rows around 64 centres (near neighbours: many distances close to a query's k-th) and queries beside rows, on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    c = torch.randn(64, d, device="cuda", generator=g)
    c /= c.norm(dim=1, keepdim=True)
    e = torch.randn(N, d, device="cuda", generator=g)
    X = c[torch.randint(0, 64, (N,), device="cuda", generator=g)] + 0.35 * e / e.norm(dim=1, keepdim=True)
    X = (X / X.norm(dim=1, keepdim=True)).float().contiguous()
    Q = X[:nq] + 0.05 * torch.randn(nq, d, device="cuda", generator=g) / (d ** 0.5)
    return X, Q.float().contiguous()


@pytest.mark.parametrize("d", [256, 512, 768, 1024])
def test_batched_search_has_the_bits_of_the_exact_scan(d):
    N = 40000
    X, Q = clustered_rows(N, d, 50 + d, nq=165)
    X[30001] = X[17]                                                     # equal rows far apart
    prep = gpu_prepare(X, N, d)
    Xb, half, norms = prep
    assert _same(Xb, X.to(torch.bfloat16).view(torch.int16))             # the copy is wise_ip_shadow_bf16's: round to nearest even
    want = 0.5 * (X.double() ** 2).sum(dim=1)
    assert float(((half.double() - want).abs() / want).max()) <= d * 2.0 ** -24      # the fixed-order fp32 sum
    assert abs(float(norms[0]) - float(X.double().norm(dim=1).max())) <= 1e-5
    again = gpu_prepare(X, N, d)
    assert all(_same(a, b) for a, b in zip(prep, again))                 # deterministic
    ids = _dev(np.random.default_rng(6).permutation(N).astype(np.int64) + 9)
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    asked = 0
    for nq in (128, 165, 3):                                             # whole passes, a ragged last pass (37 or 101 queries), the fewest
        for k in (10, 128):
            De, Ie = gpu_topk(X, N, d, Q[:nq], k, ids=ids)
            D, I = gpu_batched(X, prep, N, d, Q[:nq], k, ids=ids, counters=counters)
            assert _same(D, De) and _same(I, Ie), (d, nq, k)
            asked += nq
    De, Ie = gpu_topk(X, N, d, Q[:7], 100, id_base=4)
    D, I = gpu_batched(X, prep, N, d, Q[:7], 100, id_base=4)            # no ids, no counters
    assert _same(D, De) and _same(I, Ie)
    # on this data every query is answered from its list: no silent fallback hides a broken collect
    assert counters.cpu().numpy().tolist() == [asked, 0]


def test_batched_search_over_rows_of_norms_spread_over_six_decades():
    """Row norms 1e-3 .. 1e3: for a query beside a short row, |x|^2 / 2 and q . x of the long rows are ~1e6 and cancel to a distance
    of ~1e-6 .. 1e6 — the half-norm and cancellation terms of the band dominate.  The exact scan's bits, whichever path answers."""
    N, d = 8192, 256
    X, Q = clustered_rows(N, d, 77, nq=40)
    g = torch.Generator(device="cuda").manual_seed(78)
    scale = 10.0 ** (torch.rand(N, 1, device="cuda", generator=g) * 6.0 - 3.0)
    X = (X * scale).contiguous()
    Q = (X[::N // 40][:40] * (1.0 + 1e-3 * torch.randn(40, 1, device="cuda", generator=g))).contiguous()
    assert float(X.norm(dim=1).min()) < 2e-3 and float(X.norm(dim=1).max()) > 5e2
    prep = gpu_prepare(X, N, d)
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    for nq, k in ((5, 10), (40, 100)):
        De, Ie = gpu_topk(X, N, d, Q[:nq], k)
        D, I = gpu_batched(X, prep, N, d, Q[:nq], k, counters=counters)
        assert _same(D, De) and _same(I, Ie), (nq, k)
    assert int(counters.sum()) == 45


def test_batched_search_with_queries_midway_between_bf16_grid_points():
    """Every query component sits exactly between two neighbouring bf16 values: the largest rounding a bf16 image can carry."""
    N, d = 8192, 512
    X, Q = clustered_rows(N, d, 79, nq=40)
    bits = Q.view(torch.int32)
    Q = ((bits & ~0xFFFF) | 0x8000).view(torch.float32).contiguous()
    qb, below = Q.to(torch.bfloat16).float(), (Q.view(torch.int32) & ~0xFFFF).view(torch.float32)
    assert bool(((Q - qb).abs() == (Q - below).abs()).all()) and bool((Q != qb).all())      # as far from either neighbour: half a bf16 ulp
    prep = gpu_prepare(X, N, d)
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    for nq, k in ((5, 10), (40, 100)):
        De, Ie = gpu_topk(X, N, d, Q[:nq], k)
        D, I = gpu_batched(X, prep, N, d, Q[:nq], k, counters=counters)
        assert _same(D, De) and _same(I, Ie), (nq, k)
    assert int(counters.sum()) == 45


def test_batched_overflow_is_redone_by_the_exact_scan():
    N, d, k = 40000, 256, 10
    X, Q = clustered_rows(N, d, 91)
    q = torch.randn(d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(92))
    Q[3] = q / q.norm()                                                  # a direction of its own: no other query sees its copies
    copies = 5000                                                        # identical rows, more than a candidate list holds (4096)
    where = torch.arange(copies, device="cuda") * 7 + 5                  # spread over the whole index
    X[where] = (Q[3] * 1.01).repeat(copies, 1)
    prep = gpu_prepare(X, N, d)
    nq = 5
    De, Ie = gpu_topk(X, N, d, Q[:nq], k)
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    D, I = gpu_batched(X, prep, N, d, Q[:nq], k, counters=counters)
    assert _same(D, De) and _same(I, Ie)
    assert counters.cpu().numpy().tolist() == [0, nq]                    # the gated exact scan answered that pass's queries
    assert Ie[3].tolist() == where[:k].tolist() and len(set(_bits(De)[3].tolist())) == 1      # equal distances: the lowest positions
    counters.zero_()                                                     # a pass without that query is answered from the lists
    D, I = gpu_batched(X, prep, N, d, Q[:3], k, counters=counters)
    assert _same(D, De[:3]) and _same(I, Ie[:3]) and counters.cpu().numpy().tolist() == [3, 0]


def test_batched_refusals_leave_the_outputs_untouched():
    lib = _lib.lib()
    N, d, nq, k = 4096, 256, 4, 10
    X, Q = clustered_rows(N, d, 13, nq=nq)
    Xb, half, norms = gpu_prepare(X, N, d)
    for shape in ((N, 20, nq, k), (N, 128, nq, k), (N, 320, nq, k), (N, d, 2, k), (N, d, nq, 129), (N - 1, d, nq, k), (1 << 31, d, nq, k)):
        assert lib.wise_l2_topk_batched_workspace_bytes(*shape) == 0, shape
    need = lib.wise_l2_topk_batched_workspace_bytes(N, d, nq, k)
    ws = torch.empty(need + 64, dtype=torch.uint8, device="cuda")
    D = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    I = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    st = _lib.stream_ptr()

    def call(rows=X.data_ptr(), xb=Xb.data_ptr(), hp=half.data_ptr(), dd=d, qp=Q.data_ptr(), wsp=ws.data_ptr(), wsn=need, n=N, nqq=nq, kk=k):
        return lib.wise_l2_topk_batched(rows, xb, hp, norms.data_ptr(), n, dd, qp, nqq, kk, 0, 0, D.data_ptr(), I.data_ptr(), 0, wsp, wsn, st)

    bad = {"short workspace": call(wsn=need - 1), "no workspace": call(wsp=0), "misaligned rows": call(rows=X.data_ptr() + 4),
           "misaligned copy": call(xb=Xb.data_ptr() + 2), "no copy": call(xb=0), "no half-norms": call(hp=0),
           "misaligned queries": call(qp=Q.data_ptr() + 4), "d = 20": call(dd=20), "nq = 2": call(nqq=2), "k = 129": call(kk=129),
           "N = 4095": call(n=N - 1)}
    bad["prepare d = 20"] = lib.wise_l2_prepare(X.data_ptr(), N, 20, Xb.data_ptr(), half.data_ptr(), norms.data_ptr(), st)
    bad["prepare no half"] = lib.wise_l2_prepare(X.data_ptr(), N, d, Xb.data_ptr(), 0, norms.data_ptr(), st)
    torch.cuda.synchronize()
    assert all(rc == WISE_E_INVALID for rc in bad.values()), bad
    assert lib.wise_last_error()
    assert bool((D == 7.0).all()) and bool((I == 7).all())
    assert call() == 0                                                   # and the good call goes through
    torch.cuda.synchronize()
    De, Ie = gpu_topk(X, N, d, Q, k)
    assert _same(D, De) and _same(I, Ie)


def test_refusals_leave_the_outputs_untouched():
    lib = _lib.lib()
    N, d, nq, k = 4096, 256, 4, 10
    X, _ = make_rows(N, d, 13)
    Xd, Q = _dev(X), _dev(make_queries(X, [], nq, 14))
    D = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    I = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    st = _lib.stream_ptr()
    ws = torch.empty(lib.wise_l2_topk_workspace_bytes(N, d, nq, k), dtype=torch.uint8, device="cuda")

    def call(rows=Xd.data_ptr(), dd=d, qp=Q.data_ptr(), wsp=ws.data_ptr(), wsn=ws.numel(), n=N, nqq=nq, kk=k):
        return lib.wise_l2_topk_f32(rows, n, dd, qp, nqq, kk, 0, 0, D.data_ptr(), I.data_ptr(), wsp, wsn, st)

    bad = {"short workspace": call(wsn=ws.numel() - 512), "no workspace": call(wsp=0), "misaligned rows": call(rows=Xd.data_ptr() + 4),
           "misaligned queries": call(qp=Q.data_ptr() + 4), "d = 20": call(dd=20), "d = 1040": call(dd=1040), "nq = 0": call(nqq=0),
           "k = 2049": call(kk=2049), "N < 0": call(n=-1)}
    pos = torch.arange(10, dtype=torch.int64, device="cuda")
    bad["n_pos > N"] = lib.wise_l2_topk_pos_f32(Xd.data_ptr(), 5, d, pos.data_ptr(), 10, Q.data_ptr(), nq, k, 0, 0, D.data_ptr(), I.data_ptr(),
                                                ws.data_ptr(), ws.numel(), st)
    torch.cuda.synchronize()
    assert all(rc == WISE_E_INVALID for rc in bad.values()), bad
    assert lib.wise_last_error()
    assert bool((D == 7.0).all()) and bool((I == 7).all())
    assert call() == 0                                                   # and the good call goes through
    torch.cuda.synchronize()
    De, Ie = gpu_topk(Xd, N, d, Q, k)
    assert _same(D, De) and _same(I, Ie)


# ------------------------------------------------------------------------------------------------------------------ (5) graph capture
def test_graph_capture_of_the_exact_and_of_the_batched_search():
    lib = _lib.lib()
    N, d, nq, k = 8192, 256, 6, 10
    X, Q = clustered_rows(N, d, 17, nq=nq)
    Xb, half, norms = prep = gpu_prepare(X, N, d)
    De, Ie = gpu_topk(X, N, d, Q, k)
    Dw, Iw = gpu_batched(X, prep, N, d, Q, k)                            # both paths have run once before the capture
    assert _same(Dw, De) and _same(Iw, Ie)
    outs = [(torch.zeros(nq, k, dtype=torch.float32, device="cuda"), torch.zeros(nq, k, dtype=torch.int64, device="cuda")) for _ in range(2)]
    wse = torch.empty(lib.wise_l2_topk_workspace_bytes(N, d, nq, k), dtype=torch.uint8, device="cuda")
    wsb = torch.empty(lib.wise_l2_topk_batched_workspace_bytes(N, d, nq, k), dtype=torch.uint8, device="cuda")
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = _lib.stream_ptr()
        _lib.check(lib.wise_l2_topk_f32(X.data_ptr(), N, d, Q.data_ptr(), nq, k, 0, 0, outs[0][0].data_ptr(), outs[0][1].data_ptr(),
                                        wse.data_ptr(), wse.numel(), st))
        _lib.check(lib.wise_l2_topk_batched(X.data_ptr(), Xb.data_ptr(), half.data_ptr(), norms.data_ptr(), N, d, Q.data_ptr(), nq, k, 0, 0,
                                            outs[1][0].data_ptr(), outs[1][1].data_ptr(), counters.data_ptr(), wsb.data_ptr(), wsb.numel(), st))
    for rep in range(2):
        for D, I in outs:
            D.zero_()
            I.zero_()
        g.replay()
        torch.cuda.synchronize()
        for D, I in outs:
            assert _same(D, De) and _same(I, Ie), rep
    assert int(counters.sum()) == 2 * nq


# ------------------------------------------------------------------------------------------------------------------ (6) the class
def test_index_class_add_adopt_remove_reconstruct():
    from wise_amd.index.flat_l2 import FlatL2Index
    from wise_amd.index.selector import IDSelectorRange, SearchParameters

    N, d = 5000, 48
    rng = np.random.default_rng(23)
    X, _ = make_rows(N, d, 24)
    ids = rng.permutation(N).astype(np.int64) + 1000
    one = FlatL2Index(d)
    one.add_with_ids(X, ids)
    chunked = FlatL2Index(d)
    for s in range(0, N, 1234):
        chunked.add_with_ids(X[s:s + 1234], ids[s:s + 1234])
    reserved = FlatL2Index(d)
    reserved.reserve(N)
    for s in range(0, N, 2000):
        reserved.add_with_ids(_dev(X[s:s + 2000]), ids[s:s + 2000])      # rows already on the device
    adopted = FlatL2Index(d).adopt(_dev(X), _dev(ids))
    Q = make_queries(X, [1], 5, 25)
    Dr, Ir = ref.topk(X, Q, 20, ids=ids)
    for idx in (one, chunked, reserved, adopted):
        Xh, ih = idx.rows_host()
        assert Xh.tobytes() == X.tobytes() and np.array_equal(ih, ids)
        assert idx.ntotal == N and idx.is_trained and idx.metric == "l2" and idx.hbm_bytes() == N * (4 * d + 8)
        D, I = idx.search(Q, 20)
        assert _same(D, Dr) and _same(I, Ir)
    assert FlatL2Index(d).adopt(_dev(X)).hbm_bytes() == N * 4 * d        # implicit ids
    sel = IDSelectorRange(1500, 2500)                                    # a selector: the scan over the selected positions
    pos = np.flatnonzero((ids >= 1500) & (ids < 2500))
    Ds, Is = one.search(Q, 20, params=SearchParameters(sel=sel))
    Dp, Ip = ref.topk_pos(X, Q, 20, pos, ids=ids)
    assert _same(Ds, Dp) and _same(Is, Ip)
    want = np.array([ids[7], ids[0], 5, ids[N - 1]], dtype=np.int64)     # reconstruct_batch: the fp32 rows, NaN for an absent id
    rec = one.reconstruct_batch(want)
    assert np.isnan(rec[2]).all() and _same(rec[[0, 1, 3]], X[[7, 0, N - 1]])
    # remove_ids: byte for byte the index that received only the kept rows
    gone = np.sort(rng.permutation(N)[:777])
    keep = np.setdiff1d(np.arange(N), gone)
    assert reserved.remove_ids(ids[gone]) == 777 and reserved.remove_ids(ids[gone]) == 0
    fresh = FlatL2Index(d)
    fresh.add_with_ids(X[keep], ids[keep])
    Xr, ir = reserved.rows_host()
    Xf, if_ = fresh.rows_host()
    assert Xr.tobytes() == Xf.tobytes() == X[keep].tobytes() and np.array_equal(ir, if_) and reserved.ntotal == N - 777
    D1, I1 = reserved.search(Q, 20)
    D2, I2 = fresh.search(Q, 20)
    D3, I3 = ref.topk(X[keep], Q, 20, ids=ids[keep])
    assert _same(D1, D2) and _same(I1, I2) and _same(D1, D3) and _same(I1, I3)
    reserved.add_with_ids(X[gone[:50]], ids[gone[:50]])                  # the reserved tensor is filled from the new end
    assert reserved.ntotal == N - 727 and reserved.rows_host()[0].tobytes() == np.concatenate([X[keep], X[gone[:50]]]).tobytes()
    assert one.remove_ids(IDSelectorRange(0, 10 ** 9)) == N and one.ntotal == 0
    D, I = one.search(Q, 3)
    assert (I == -1).all() and (D == PAD).all()
    with pytest.raises(ValueError, match="multiple of 16"):
        FlatL2Index(40)


def test_index_class_routes_batches_to_the_matrix_cores():
    from wise_amd.index.flat_l2 import FlatL2Index
    from wise_amd.index.flat_sq import FlatSQfp16IPIndex

    N, d = 12000, 512
    X, Q = clustered_rows(N, d, 29, nq=40)
    ids = _dev(np.arange(N, dtype=np.int64) * 2)
    idx = FlatL2Index(d).adopt(X, ids)
    assert FlatL2Index.BATCH_MIN_ROWS == FlatSQfp16IPIndex.BATCH_MIN_ROWS == 1 << 18       # the provisional floors: IndexSQfp16's
    assert FlatL2Index.BATCH_MIN_QUERIES == FlatSQfp16IPIndex.BATCH_MIN_QUERIES == 8
    De, Ie = idx.search_device(Q, 10)                                    # under the row floor: the exact scan, no copy built
    assert idx.batched_counts() == (0, 0) and idx._Xb is None and idx.hbm_bytes() == N * (4 * d + 8)
    idx.BATCH_MIN_ROWS = 4096
    D, I = idx.search_device(Q, 10)
    assert idx.batched_counts() == (40, 0) and _same(D, De) and _same(I, Ie) and idx._Xb is not None and idx._half.shape == (N,)
    D2, I2 = idx.search_device(Q[:2], 10)                                # two queries: no batched shape
    assert sum(idx.batched_counts()) == 40 and _same(D2, De[:2]) and _same(I2, Ie[:2])
    D7, I7 = idx.search_device(Q[:7], 10)                                # under the query floor: the exact scan's passes
    assert sum(idx.batched_counts()) == 40 and _same(D7, De[:7]) and _same(I7, Ie[:7])
    D8, I8 = idx.search_device(Q[:8], 10)
    assert sum(idx.batched_counts()) == 48 and _same(D8, De[:8]) and _same(I8, Ie[:8])
    D3, I3 = idx.search_device(Q, 200)                                   # k > 128: the exact scan
    assert sum(idx.batched_counts()) == 48 and _same(I3[:, :10], Ie)
    # the copy and the half-norms go with the rows: an add drops them, the next batch rebuilds them over all rows
    extra = (Q[:5] * 1.0001).contiguous()
    idx.add_with_ids(extra, np.arange(5, dtype=np.int64) + 10 ** 6)
    assert idx._Xb is None and idx._half is None and idx._norms is None
    Dn, In = idx.search_device(Q, 10)
    assert idx._Xb.shape == (N + 5, d) and sum(idx.batched_counts()) == 88
    fresh = FlatL2Index(d).adopt(torch.cat([X, extra]), torch.cat([ids, _dev(np.arange(5, dtype=np.int64) + 10 ** 6)]))
    Df, If = fresh.search_device(Q, 10)                                  # under the row floor: the exact scan
    assert _same(Dn, Df) and _same(In, If) and (In[:5, 0] >= 10 ** 6).all()


# ------------------------------------------------------------------------------------------------------------------ (7) sharding
@pytest.mark.parametrize("W", [1, 3, 8])
def test_slices_merged_in_rank_order_are_the_whole_index(W):
    from wise_amd.index.flat_l2 import FlatL2Index

    N, d, nq = 6001, 48, 4
    X, dup = make_rows(N, d, 61)
    for r in range(1, W):                                                # equal rows on both sides of every slice boundary
        lo = shard_range(N, r, W)[0]
        X[lo] = X[lo - 1]
        dup.append(lo - 1)
    Q = make_queries(X, dup[-3:], nq, 12)
    ids = np.random.default_rng(7).permutation(N).astype(np.int64) + 1
    whole = FlatL2Index(d).adopt(_dev(X), _dev(ids))
    for k in (1, 10, 100):
        De, Ie = whole.search_device(_dev(Q), k)
        Dr, Ir = ref.topk(X, Q, k, ids=ids)
        assert _same(De, Dr) and _same(Ie, Ir)
        Ds, Is = [], []
        for r in range(W):
            lo, hi = shard_range(N, r, W)
            part = FlatL2Index(d).adopt(_dev(X[lo:hi]), _dev(ids[lo:hi]))
            D, I = part.search_device(_dev(Q), k)
            Ds.append(-D)                                                # what the wrapper exchanges: the negated distances
            Is.append(I)
        D, I = merge_device(torch.stack(Ds), torch.stack(Is), k)
        assert _same(-D, De) and _same(I, Ie), (W, k)


def test_sharded_plugin_over_rccl_world1(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "sharded_flat_l2_nccl_worker.py"), str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert res["ok"], json.dumps(res)
    assert res["exchange_bytes"] == 16 * 3 * 10                          # one exchange of (score, id) planes: nq = 3, k = 10

"""-m gpu: IndexSQ8bit (csrc/ip_sq8.hip, wise_amd/index/flat_sq.py: FlatSQ8IPIndex) — every path bit for bit against
tests/sq8_flat_ref.py, or, for the batched search, against wise_ipsq8_topk on the same data.

(1) encode, wise_sq_minmax, reconstruct and prepare; (2) the exact scan over shapes that take every path of it (rows per wave-load
    64 .. 1, C = 3 with idle lanes, 1 / 2 / 4 queries a pass, list lengths, several blocks and a ragged tail), duplicate rows, and
    scores that the final addition rounds together; (3) the scan over positions and range count / fill; (4) the batched search, its
    constructed overflow, its scaling and its refusals; (5) graph capture; (6) the index class; (7) the plugin's files, slices
    merged in rank order, and the plugin on RCCL."""
import hashlib
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import sq8_flat_ref as ref
from wise_amd import _lib
from wise_amd.index.sharded import merge_device, shard_range

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
WISE_E_INVALID = -1
NEG = np.float32(-3.4028234663852886e38)
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
    """(codes [N,d] uint8, vmin, vdiff, X, rows whose copies exist): ranges over every row, a duplicate pair on both sides of a block
    boundary and one at the two ends."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((max(N, 1), d)).astype(np.float32) / np.float32(np.sqrt(d))
    dup = []
    B = block_rows(d)
    if N > B + 1:
        X[B - 1] *= np.float32(4.0)                                      # long rows: under their own direction no other row comes near
        X[B] = X[B - 1]
        dup.append(B - 1)
    if N > 2:
        X[1] *= np.float32(4.0)
        X[N - 1] = X[1]
        dup.append(1)
    vmin, vdiff = ref.train(X)
    X = X[:N]
    return ref.encode(X, vmin, vdiff), vmin, vdiff, X, dup


def make_queries(X, dup, nq, seed):
    Q = np.random.default_rng(seed).standard_normal((nq, X.shape[1])).astype(np.float32)
    for i, r in enumerate(dup[:nq]):
        Q[i] = X[r] * np.float32(3.0)                                    # its copies share the best score
    return Q


def gpu_topk(Cd, Td, N, d, Qd, k, ids=None, id_base=0, pos=None):
    lib = _lib.lib()
    nq = Qd.shape[0]
    D = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    I = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    n_items = N if pos is None else pos.numel()
    need = lib.wise_ipsq8_topk_workspace_bytes(n_items, d, nq, k)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    if pos is None:
        rc = lib.wise_ipsq8_topk(_lib.ptr(Cd), Td.data_ptr(), N, d, Qd.data_ptr(), nq, k, _lib.ptr(ids), id_base, D.data_ptr(),
                                 I.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    else:
        rc = lib.wise_ipsq8_topk_pos(_lib.ptr(Cd), Td.data_ptr(), N, d, _lib.ptr(pos), pos.numel(), Qd.data_ptr(), nq, k, _lib.ptr(ids),
                                     id_base, D.data_ptr(), I.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "wise_ipsq8_topk")
    return D, I


def _trained(vmin, vdiff):
    return _dev(np.concatenate([vmin, vdiff]).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ (1) the codec
def test_encode_minmax_reconstruct_and_prepare_bit_for_bit():
    lib = _lib.lib()
    st = _lib.stream_ptr()
    N, d = 3001, 48
    rng = np.random.default_rng(1)
    X = rng.standard_normal((N, d)).astype(np.float32)
    X[:, 5] = np.float32(0.25)                                           # a dimension with vdiff == 0
    vmin, vdiff = ref.train(X[:2000])                                    # the rest holds values outside the ranges: they clamp
    assert vdiff[5] == 0 and (X[2000:] < vmin).any() and (X[2000:] > vmin + vdiff).any()
    Xd, Td = _dev(X), _trained(vmin, vdiff)
    codes = torch.full((N, d), 9, dtype=torch.uint8, device="cuda")
    _lib.check(lib.wise_sq_encode(Xd.data_ptr(), Td.data_ptr(), N, d, codes.data_ptr(), st), "wise_sq_encode")
    C = ref.encode(X, vmin, vdiff)
    assert _same(codes, C) and (C[2000:] == 0).any() and (C[2000:] == 255).any() and (C[:, 5] == 0).all()
    # wise_sq_minmax over ragged chunks == wise_sq_train over all rows
    T = torch.empty(2 * d, dtype=torch.float32, device="cuda")
    _lib.check(lib.wise_sq_train(Xd.data_ptr(), N, d, T.data_ptr(), st), "wise_sq_train")
    lo = torch.full((d,), 5.0, dtype=torch.float32, device="cuda")
    hi = torch.full((d,), -5.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.wise_sq_minmax(0, 0, d, lo.data_ptr(), hi.data_ptr(), 0, st), "wise_sq_minmax")      # no rows: +max / -max
    assert bool((lo == 3.4028234663852886e38).all()) and bool((hi == -3.4028234663852886e38).all())
    for a, b in ((0, 1), (1, 7), (7, 7), (7, 1500), (1500, N)):
        _lib.check(lib.wise_sq_minmax(Xd[a:].data_ptr(), b - a, d, lo.data_ptr(), hi.data_ptr(), 1, st), "wise_sq_minmax")
    va, vd = ref.train(X)
    assert _same(lo, va) and _same(hi - lo, vd) and _same(T[:d], va) and _same(T[d:], vd)
    lo2, hi2 = torch.empty_like(lo), torch.empty_like(hi)
    _lib.check(lib.wise_sq_minmax(Xd.data_ptr(), N, d, lo2.data_ptr(), hi2.data_ptr(), 0, st), "wise_sq_minmax")   # one chunk, fresh
    assert _same(lo2, lo) and _same(hi2, hi)
    # reconstruct: ivfsq_ref.decode, NaN rows for ids nobody carries; the highest position where an id repeats
    ids = np.arange(N, dtype=np.int64) * 3 + 1
    ids[77] = ids[5]
    want = np.array([ids[0], ids[5], 2, ids[N - 1], -4], dtype=np.int64)
    out = torch.zeros(len(want), d, dtype=torch.float32, device="cuda")
    idd, wd = _dev(ids), _dev(want)
    _lib.check(lib.wise_ipsq8_reconstruct(codes.data_ptr(), Td.data_ptr(), N, d, idd.data_ptr(), 0, wd.data_ptr(), len(want),
                                          out.data_ptr(), st), "wise_ipsq8_reconstruct")
    R = ref.reconstruct(C, vmin, vdiff, ids, want)
    got = out.cpu().numpy()
    assert np.isnan(R[[2, 4]]).all() and np.isnan(got[[2, 4]]).all()
    assert _same(got[[0, 1, 3]], R[[0, 1, 3]]) and _same(got[1], ref.decode(C[77:78], vmin, vdiff)[0])
    _lib.check(lib.wise_ipsq8_reconstruct(codes.data_ptr(), Td.data_ptr(), N, d, 0, 10, wd.data_ptr(), len(want), out.data_ptr(), st),
               "wise_ipsq8_reconstruct")                                # implicit ids: id_base + row
    got, R = out.cpu().numpy(), ref.reconstruct(C, vmin, vdiff, None, want - 10)
    assert np.array_equal(np.isnan(got), np.isnan(R)) and _same(got[~np.isnan(R)], R[~np.isnan(R)]) and not np.isnan(R[1]).any()
    # prepare
    norms = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.wise_ipsq8_prepare(codes.data_ptr(), N, d, norms.data_ptr(), st), "wise_ipsq8_prepare")
    assert _same(norms, np.array([ref.code_norm(C)], np.float32))
    _lib.check(lib.wise_ipsq8_prepare(0, 0, d, norms.data_ptr(), st), "wise_ipsq8_prepare")
    assert float(norms[0]) == 0.0


# ------------------------------------------------------------------------------------------------------------------ (2) exact scan
@pytest.mark.parametrize("d", [16, 48, 128, 512, 1024])
@pytest.mark.parametrize("N", [0, 1, 63, 2049, 6000])
def test_exact_scan_bit_for_bit(d, N):
    C, vmin, vdiff, X, dup = make_rows(N, d, 100 + d + N)
    Q = make_queries(X, dup, 5, 7) if N else np.random.default_rng(7).standard_normal((5, d)).astype(np.float32)
    S = ref.scores(C, vmin, vdiff, Q)                                    # once per shape, shared by every case below
    ids = np.random.default_rng(1).permutation(N).astype(np.int64) * 3 + 11
    Cd, Td, Qd, idd = _dev(C).reshape(N, d), _trained(vmin, vdiff), _dev(Q), _dev(ids)
    if N > block_rows(d) + 1:                                            # the duplicates: equal scores, the lower position first
        D, I = gpu_topk(Cd, Td, N, d, Qd[:1], 10)
        I = I.cpu().numpy()[0]
        at = list(I).index(block_rows(d) - 1)
        assert I[at + 1] == block_rows(d) and _bits(D)[0, at] == _bits(D)[0, at + 1]
    for nq in (1, 2, 3, 5):
        for k in (1, 10, 100, 2048):
            Dr, Ir = ref.topk(S[:nq], k, id_base=5)
            D, I = gpu_topk(Cd, Td, N, d, Qd[:nq], k, id_base=5)
            assert _same(D, Dr) and _same(I, Ir), (d, N, nq, k, "positions")
            Dr, Ir = ref.topk(S[:nq], k, ids=ids)
            D, I = gpu_topk(Cd, Td, N, d, Qd[:nq], k, ids=idd)
            assert _same(D, Dr) and _same(I, Ir), (d, N, nq, k, "ids")
            if N < k:                                                    # padding
                assert (Ir[:, N:] == -1).all() and (Dr[:, N:] == NEG).all()


def test_final_addition_rounds_different_sums_to_one_score():
    """q0 is large beside the rows' sums: rows whose s_0 differ get the same fl(q0 + s_0), and the lower position wins among them —
    the keys are on the final sum, not on s_0."""
    N, d = 500, 16
    rng = np.random.default_rng(3)
    vmin = np.full(d, 1000.0, np.float32)
    vdiff = np.full(d, 0.01, np.float32)
    C = rng.integers(100, 104, size=(N, d)).astype(np.uint8)
    Q = np.ones((2, d), np.float32)
    Q[1] = -1.0
    W, q0 = ref.query(Q, vmin, vdiff)
    S = ref.scores(C, vmin, vdiff, Q)
    s0 = ref.row_sums(C, W[0])
    assert len(np.unique(s0)) > 20 and len(np.unique(S[0])) < len(np.unique(s0))      # different sums, fewer scores
    best = np.flatnonzero(S[0] == S[0].max())
    assert len(best) > 1 and len(np.unique(s0[best])) > 1
    Cd, Td, Qd = _dev(C), _trained(vmin, vdiff), _dev(Q)
    for k in (1, 10, 500):
        Dr, Ir = ref.topk(S, k)
        D, I = gpu_topk(Cd, Td, N, d, Qd, k)
        assert _same(D, Dr) and _same(I, Ir), k
    assert int(gpu_topk(Cd, Td, N, d, Qd[:1], 1)[1][0, 0]) == int(best[0])


def test_exact_scan_several_blocks_and_a_ragged_tail():
    d, N = 16, 70001
    assert N > 4 * block_rows(d) and N % (64 // (d // 16)) != 0
    C, vmin, vdiff, X, dup = make_rows(N, d, 5)
    Q = make_queries(X, dup, 5, 8)
    S = ref.scores(C, vmin, vdiff, Q)
    Cd, Td, Qd = _dev(C), _trained(vmin, vdiff), _dev(Q)
    for nq, k in ((1, 10), (5, 100), (4, 1024), (2, 2048)):
        Dr, Ir = ref.topk(S[:nq], k)
        D, I = gpu_topk(Cd, Td, N, d, Qd[:nq], k)
        assert _same(D, Dr) and _same(I, Ir), (nq, k)
    I = gpu_topk(Cd, Td, N, d, Qd[:2], 10)[1].cpu().numpy()
    assert list(I[0]).index(block_rows(d) - 1) + 1 == list(I[0]).index(block_rows(d))      # across a block boundary
    assert list(I[1]).index(1) + 1 == list(I[1]).index(N - 1)                             # across the whole grid


# ------------------------------------------------------------------------------------------------------------------ (3) positions, range
@pytest.mark.parametrize("d", [48, 512])
def test_position_scan_equals_the_restatement_restricted(d):
    N = 6000
    C, vmin, vdiff, X, dup = make_rows(N, d, 31 + d)
    Q = make_queries(X, dup, 5, 9)
    S = ref.scores(C, vmin, vdiff, Q)
    ids = np.arange(N, dtype=np.int64) * 2 + 1
    Cd, Td, Qd, idd = _dev(C), _trained(vmin, vdiff), _dev(Q), _dev(ids)
    rng = np.random.default_rng(2)
    sets = {"empty": np.zeros(0, np.int64), "one": np.array([block_rows(d)], np.int64), "every": np.arange(N, dtype=np.int64),
            "sparse": np.sort(rng.permutation(N)[:137]).astype(np.int64),
            "dups": np.array([1, block_rows(d) - 1, block_rows(d), N - 1], np.int64)}
    for name, pos in sets.items():
        pd = _dev(pos) if pos.size else torch.zeros(0, dtype=torch.int64, device="cuda")
        for nq in (1, 5):
            for k in (1, 10, 100):
                Dr, Ir = ref.topk_pos(S[:nq], k, pos, ids=ids)
                D, I = gpu_topk(Cd, Td, N, d, Qd[:nq], k, ids=idd, pos=pd)
                assert _same(D, Dr) and _same(I, Ir), (name, nq, k)
                if name == "every":
                    Da, Ia = gpu_topk(Cd, Td, N, d, Qd[:nq], k, ids=idd)
                    assert _same(D, Da) and _same(I, Ia)
        Dr, Ir = ref.topk_pos(S[:2], 10, pos, id_base=3)
        D, I = gpu_topk(Cd, Td, N, d, Qd[:2], 10, id_base=3, pos=pd)
        assert _same(D, Dr) and _same(I, Ir), name


def _index(d, C, vmin, vdiff, ids=None, id_base=0):
    from wise_amd.index.flat_sq import FlatSQ8IPIndex
    idx = FlatSQ8IPIndex(d)
    idx.set_trained(vmin, vdiff)
    return idx.adopt(C if torch.is_tensor(C) else _dev(C), None if ids is None else _dev(ids), id_base)


@pytest.mark.parametrize("d", [16, 512])
def test_range_search_is_the_prefix_of_the_exact_scan(d):
    from wise_amd.index.selector import IDSelectorBatch

    N, nq = 6000, 5
    C, vmin, vdiff, X, dup = make_rows(N, d, 41 + d)
    Q = make_queries(X, dup, nq, 10)
    S = ref.scores(C, vmin, vdiff, Q)
    ids = np.random.default_rng(3).permutation(N).astype(np.int64) + 100
    idx = _index(d, C, vmin, vdiff, ids)
    D2k, I2k = gpu_topk(idx._codes_t, idx._trained, N, d, _dev(Q), 2048, ids=idx._ids)
    D2k, I2k = D2k.cpu().numpy(), I2k.cpu().numpy()
    chosen = np.sort(np.random.default_rng(4).permutation(ids)[:N // 3])
    keep = np.isin(ids, chosen)
    kth = np.sort(S, axis=1)
    above = float(np.nextafter(S.max(), np.float32(np.inf)))            # one above every score
    for thr in (float(kth[:, -40].max()), float(kth[:, -1500].min()), float(S.max()), above, float(NEG)):    # few, many, none, none, every row
        for sel, mask in ((None, None), (IDSelectorBatch(chosen), keep)):
            lims, D, I = (t.cpu().numpy() for t in idx.range_search_device(_dev(Q), thr, sel=sel, chunk=2))
            lr, Dr, Ir = ref.range_search(S, thr, ids=ids, keep=mask)
            assert np.array_equal(lims, lr) and _same(D, Dr) and _same(I, Ir), (d, thr, sel is not None)
            if mask is None:                                             # the check of tests/test_gpu_range.py: a prefix of the top-2048
                for q in range(nq):
                    n = min(int(lims[q + 1] - lims[q]), 2048)
                    assert _same(D[lims[q]:lims[q] + n], D2k[q, :n]) and _same(I[lims[q]:lims[q] + n], I2k[q, :n])
    lims, D, I = idx.range_search(Q, above)
    assert lims.tolist() == [0] * (nq + 1) and D.size == 0 and I.size == 0
    lims, _, _ = idx.range_search(Q[:1], float(NEG))
    assert lims.tolist() == [0, N]
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            idx.range_search(Q, bad)


# ------------------------------------------------------------------------------------------------------------------ (4) batched
def gpu_batched(Cd, Td, norms, N, d, Qd, k, ids=None, id_base=0, counters=None):
    lib = _lib.lib()
    nq = Qd.shape[0]
    D = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    I = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    need = lib.wise_ipsq8_topk_batched_workspace_bytes(N, d, nq, k)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _lib.check(lib.wise_ipsq8_topk_batched(Cd.data_ptr(), Td.data_ptr(), norms.data_ptr(), N, d, Qd.data_ptr(), nq, k, _lib.ptr(ids),
                                           id_base, D.data_ptr(), I.data_ptr(), _lib.ptr(counters), ws.data_ptr(), ws.numel(),
                                           _lib.stream_ptr()), "wise_ipsq8_topk_batched")
    return D, I


def prepare(Cd, N, d):
    norms = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().wise_ipsq8_prepare(Cd.data_ptr(), N, d, norms.data_ptr(), _lib.stream_ptr()), "wise_ipsq8_prepare")
    return norms


def clustered_codes(N, d, seed):
    """unit rows around 64 centres (near neighbours: many scores close to a query's k-th), trained over every row and encoded on the
    device: (codes [N,d] uint8, trained [2d], queries [130,d])"""
    lib = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(seed)
    c = torch.randn(64, d, device="cuda", generator=g)
    c /= c.norm(dim=1, keepdim=True)
    e = torch.randn(N, d, device="cuda", generator=g)
    X = c[torch.randint(0, 64, (N,), device="cuda", generator=g)] + 0.35 * e / e.norm(dim=1, keepdim=True)
    X = (X / X.norm(dim=1, keepdim=True)).contiguous()
    Q = X[:130] + 0.05 * torch.randn(130, d, device="cuda", generator=g) / (d ** 0.5)
    T = torch.empty(2 * d, dtype=torch.float32, device="cuda")
    C = torch.empty(N, d, dtype=torch.uint8, device="cuda")
    _lib.check(lib.wise_sq_train(X.data_ptr(), N, d, T.data_ptr(), _lib.stream_ptr()), "wise_sq_train")
    _lib.check(lib.wise_sq_encode(X.data_ptr(), T.data_ptr(), N, d, C.data_ptr(), _lib.stream_ptr()), "wise_sq_encode")
    return C, T, Q.float().contiguous()


@pytest.mark.parametrize("d", [256, 512, 768, 1024])
def test_batched_search_has_the_bits_of_the_exact_scan(d):
    C, T, Q = clustered_codes(40000, d, 50 + d)
    C[30001] = C[17]                                                     # equal rows far apart
    ids = _dev(np.random.default_rng(6).permutation(40000).astype(np.int64) + 9)
    for N in (4096, 5000, 40000):                                        # the first N rows: 128 groups, a ragged last group, the whole set
        Cn = C[:N]
        norms = prepare(Cn, N, d)
        want = float(Cn.float().norm(dim=1).max())
        assert abs(float(norms[0]) - want) <= 1e-5 * want and _same(prepare(Cn, N, d), norms)      # deterministic
        counters = torch.zeros(2, dtype=torch.int32, device="cuda")
        asked = 0
        for nq in (3, 33, 65, 129):                                      # query tiles 1, 2, 4 and a second pass
            for k in (1, 10, 128):
                De, Ie = gpu_topk(Cn, T, N, d, Q[:nq], k, ids=ids)
                D, I = gpu_batched(Cn, T, norms, N, d, Q[:nq], k, ids=ids, counters=counters)
                assert _same(D, De) and _same(I, Ie), (d, N, nq, k)
                asked += nq
        De, Ie = gpu_topk(Cn, T, N, d, Q[:7], 100, id_base=4)
        D, I = gpu_batched(Cn, T, norms, N, d, Q[:7], 100, id_base=4)   # no ids, no counters
        assert _same(D, De) and _same(I, Ie)
        c = counters.cpu().numpy()
        assert int(c[0]) == asked and int(c[1]) == 0, (N, c)             # on the clustered rows every query is answered from its list


def test_batched_search_scales_the_query_image_by_a_power_of_two():
    """Queries scaled by 1e4 and by 1e-6: unscaled, the weights W = q vdiff / 255 of the small ones lie below binary16's normal range
    (all of them below 2^-24 would round to zero) and the large ones lose nothing; the per-query power of two makes either case the
    ordinary one, and the lists still answer."""
    N, d = 8192, 256
    C, T, Q = clustered_codes(N, d, 77)
    norms = prepare(C, N, d)
    W = (Q[:40] * T[d:]) / 255.0
    assert float((W * 1e-6).abs().max()) < 2.0 ** -24
    for scale in (1e4, 1e-6):
        Qs = (Q * scale).contiguous()
        counters = torch.zeros(2, dtype=torch.int32, device="cuda")
        for nq, k in ((5, 10), (40, 100)):
            De, Ie = gpu_topk(C, T, N, d, Qs[:nq], k)
            D, I = gpu_batched(C, T, norms, N, d, Qs[:nq], k, counters=counters)
            assert _same(D, De) and _same(I, Ie), (scale, nq, k)
        assert counters.cpu().numpy().tolist() == [45, 0], scale
    # weights that cannot be scaled into binary16 (the largest below 2^-112), and a query that is not finite: the exact scan answers
    Qt = (Q[:6] * 1e-36).contiguous()
    Qt[4, 3] = float("inf")
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    De, Ie = gpu_topk(C, T, N, d, Qt[:4], 10)
    D, I = gpu_batched(C, T, norms, N, d, Qt[:4], 10, counters=counters)
    assert _same(D, De) and _same(I, Ie) and counters.cpu().numpy().tolist() == [0, 4]
    De, Ie = gpu_topk(C, T, N, d, Qt, 10)
    D, I = gpu_batched(C, T, norms, N, d, Qt, 10, counters=counters)
    assert _same(D, De) and _same(I, Ie) and counters.cpu().numpy().tolist() == [0, 10]


def test_batched_overflow_is_redone_by_the_exact_scan():
    N, d, k = 40000, 256, 10
    C, T, Q = clustered_codes(N, d, 91)
    q = torch.randn(d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(92))
    Q[3] = q / q.norm()                                                  # a direction of its own: no other query sees its copies
    row = torch.where(Q[3] > 0, 255, 0).to(torch.uint8)                  # the best row there is for it, 6000 times: a list holds 4096
    copies = 6000
    where = torch.arange(copies, device="cuda") * 6 + 5                  # spread over the whole index
    C[where] = row
    norms = prepare(C, N, d)
    nq = 5
    De, Ie = gpu_topk(C, T, N, d, Q[:nq], k)
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    D, I = gpu_batched(C, T, norms, N, d, Q[:nq], k, counters=counters)
    assert _same(D, De) and _same(I, Ie)
    c = counters.cpu().numpy()
    assert c[1] > 0 and int(c.sum()) == nq, c                            # the fallback ran, every query counted once
    assert Ie[3].tolist() == where[:k].tolist()                          # the copies are that query's answer, the lower positions first
    counters.zero_()
    D, I = gpu_batched(C, T, norms, N, d, Q[:3], k, counters=counters)  # a pass without that query is answered from the lists
    assert _same(D, De[:3]) and _same(I, Ie[:3]) and counters.cpu().numpy().tolist() == [3, 0]


def test_batched_refusals_leave_the_outputs_untouched():
    lib = _lib.lib()
    N, d, nq, k = 4096, 256, 4, 10
    C, T, Q = clustered_codes(N, d, 13)
    Q = Q[:nq].contiguous()
    norms = prepare(C, N, d)
    for shape in ((N, 20, nq, k), (N, 128, nq, k), (N, 320, nq, k), (N, d, 2, k), (N, d, nq, 129), (N - 1, d, nq, k)):
        assert lib.wise_ipsq8_topk_batched_workspace_bytes(*shape) == 0, shape
    need = lib.wise_ipsq8_topk_batched_workspace_bytes(N, d, nq, k)
    ws = torch.empty(need + 64, dtype=torch.uint8, device="cuda")
    D = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    I = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    st = _lib.stream_ptr()

    def call(rows=C.data_ptr(), tr=T.data_ptr(), dd=d, qp=Q.data_ptr(), wsp=ws.data_ptr(), wsn=need, n=N, nqq=nq, kk=k):
        return lib.wise_ipsq8_topk_batched(rows, tr, norms.data_ptr(), n, dd, qp, nqq, kk, 0, 0, D.data_ptr(), I.data_ptr(), 0, wsp, wsn, st)

    bad = {"short workspace": call(wsn=need - 1), "no workspace": call(wsp=0), "misaligned codes": call(rows=C.data_ptr() + 2),
           "misaligned queries": call(qp=Q.data_ptr() + 4), "misaligned workspace": call(wsp=ws.data_ptr() + 4, wsn=need + 32),
           "no ranges": call(tr=0), "d = 20": call(dd=20), "nq = 2": call(nqq=2), "k = 129": call(kk=129), "N = 4095": call(n=N - 1)}
    torch.cuda.synchronize()
    assert all(rc == WISE_E_INVALID for rc in bad.values()), bad
    assert lib.wise_last_error()
    assert bool((D == 7.0).all()) and bool((I == 7).all())
    # the exact scan's own refusals
    wse = torch.empty(lib.wise_ipsq8_topk_workspace_bytes(N, d, nq, k), dtype=torch.uint8, device="cuda")
    t = T.data_ptr()
    for rc in (lib.wise_ipsq8_topk(C.data_ptr(), t, N, 20, Q.data_ptr(), nq, k, 0, 0, D.data_ptr(), I.data_ptr(), wse.data_ptr(), wse.numel(), st),
               lib.wise_ipsq8_topk(C.data_ptr() + 2, t, N, d, Q.data_ptr(), nq, k, 0, 0, D.data_ptr(), I.data_ptr(), wse.data_ptr(), wse.numel(), st),
               lib.wise_ipsq8_topk(C.data_ptr(), 0, N, d, Q.data_ptr(), nq, k, 0, 0, D.data_ptr(), I.data_ptr(), wse.data_ptr(), wse.numel(), st),
               lib.wise_ipsq8_topk(C.data_ptr(), t, N, d, Q.data_ptr(), nq, k, 0, 0, D.data_ptr(), I.data_ptr(), wse.data_ptr(), wse.numel() - 512, st),
               lib.wise_ipsq8_topk(C.data_ptr(), t, N, d, Q.data_ptr(), nq, 2049, 0, 0, D.data_ptr(), I.data_ptr(), wse.data_ptr(), wse.numel(), st)):
        assert rc == WISE_E_INVALID
    torch.cuda.synchronize()
    assert bool((D == 7.0).all()) and bool((I == 7).all())
    assert call() == 0                                                   # and the good call goes through
    torch.cuda.synchronize()
    De, Ie = gpu_topk(C, T, N, d, Q, k)
    assert _same(D, De) and _same(I, Ie)


# ------------------------------------------------------------------------------------------------------------------ (5) graph capture
def test_graph_capture_of_the_exact_and_of_the_batched_search():
    lib = _lib.lib()
    N, d, nq, k = 8192, 256, 6, 10
    C, T, Q = clustered_codes(N, d, 17)
    Q = Q[:nq].contiguous()
    norms = prepare(C, N, d)
    De, Ie = gpu_topk(C, T, N, d, Q, k)
    Dw, Iw = gpu_batched(C, T, norms, N, d, Q, k)                        # both paths have run once before the capture
    assert _same(Dw, De) and _same(Iw, Ie)
    outs = [(torch.zeros(nq, k, dtype=torch.float32, device="cuda"), torch.zeros(nq, k, dtype=torch.int64, device="cuda")) for _ in range(2)]
    wse = torch.empty(lib.wise_ipsq8_topk_workspace_bytes(N, d, nq, k), dtype=torch.uint8, device="cuda")
    wsb = torch.empty(lib.wise_ipsq8_topk_batched_workspace_bytes(N, d, nq, k), dtype=torch.uint8, device="cuda")
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = _lib.stream_ptr()
        _lib.check(lib.wise_ipsq8_topk(C.data_ptr(), T.data_ptr(), N, d, Q.data_ptr(), nq, k, 0, 0, outs[0][0].data_ptr(),
                                       outs[0][1].data_ptr(), wse.data_ptr(), wse.numel(), st))
        _lib.check(lib.wise_ipsq8_topk_batched(C.data_ptr(), T.data_ptr(), norms.data_ptr(), N, d, Q.data_ptr(), nq, k, 0, 0,
                                               outs[1][0].data_ptr(), outs[1][1].data_ptr(), counters.data_ptr(), wsb.data_ptr(),
                                               wsb.numel(), st))
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
def test_index_class_train_add_adopt_remove_reconstruct():
    from wise_amd.index.flat_sq import FlatSQ8IPIndex
    from wise_amd.index.selector import IDSelectorRange, SearchParameters

    N, d = 5000, 48
    rng = np.random.default_rng(23)
    X = (rng.standard_normal((N, d)) / np.sqrt(d)).astype(np.float32)
    ids = rng.permutation(N).astype(np.int64) + 1000
    vmin, vdiff = ref.train(X)
    C = ref.encode(X, vmin, vdiff)
    one = FlatSQ8IPIndex(d)
    assert not one.is_trained
    for early in (lambda: one.add_with_ids(X, ids), lambda: one.add_codes_with_ids(C, ids), lambda: one.search(X[:1], 3)):
        with pytest.raises(RuntimeError, match="before train"):
            early()
    one.train(X)
    assert one.is_trained and _same(np.concatenate(one.trained_host()), np.concatenate([vmin, vdiff]))
    one.add_with_ids(X, ids)
    with pytest.raises(RuntimeError, match="cannot change"):
        one.train(X)
    chunked = FlatSQ8IPIndex(d)
    chunked.ENCODE_BYTES = 4 * d * 300                                   # the staging: 300 rows at a time, for the ranges and the codes
    chunked.train(X)
    for s in range(0, N, 1234):
        chunked.add_with_ids(X[s:s + 1234], ids[s:s + 1234])
    staged = FlatSQ8IPIndex(d)                                           # trained from staged chunks, rows already on the device
    lohi = None
    for s in range(0, N, 2000):
        lohi = staged.minmax(_dev(X[s:s + 2000]), lohi)
    staged.set_minmax(lohi)
    staged.reserve(N)
    for s in range(0, N, 2000):
        staged.add_with_ids(_dev(X[s:s + 2000]), ids[s:s + 2000])
    adopted = FlatSQ8IPIndex(d)
    adopted.set_trained(vmin, vdiff)
    adopted.adopt(_dev(C), _dev(ids))
    loaded = FlatSQ8IPIndex(d)
    loaded.set_trained(vmin, vdiff)
    loaded.reserve(N)
    loaded.add_codes_with_ids(C[:3000], ids[:3000])
    loaded.add_codes_with_ids(C[3000:], ids[3000:])
    Q = rng.standard_normal((5, d)).astype(np.float32)
    S = ref.scores(C, vmin, vdiff, Q)
    Dr, Ir = ref.topk(S, 20, ids=ids)
    for idx in (one, chunked, staged, adopted, loaded):
        Ch, ih = idx.rows_host()
        assert Ch.dtype == np.uint8 and Ch.tobytes() == C.tobytes() and np.array_equal(ih, ids)
        assert _same(np.concatenate(idx.trained_host()), np.concatenate([vmin, vdiff]))
        assert idx.ntotal == N and idx.is_trained and idx.hbm_bytes() == N * (d + 8) + 8 * d
        assert idx._codes_t.dtype == torch.uint8 and not hasattr(idx, "_X")      # no fp32 rows, no shadow
        D, I = idx.search(Q, 20)
        assert _same(D, Dr) and _same(I, Ir)
    # values outside the trained ranges clamp, as in IndexIVFSQ8
    wide = FlatSQ8IPIndex(d)
    wide.set_trained(vmin, vdiff)
    wide.add_with_ids(X * np.float32(3.0), ids)
    Cw = wide.rows_host()[0]
    assert Cw.tobytes() == ref.encode(X * np.float32(3.0), vmin, vdiff).tobytes() and (Cw == 0).any() and (Cw == 255).any()
    # a selector: the scan over the selected positions
    sel = IDSelectorRange(1500, 2500)
    pos = np.flatnonzero((ids >= 1500) & (ids < 2500))
    Ds, Is = one.search(Q, 20, params=SearchParameters(sel=sel))
    Dp, Ip = ref.topk_pos(S, 20, pos, ids=ids)
    assert _same(Ds, Dp) and _same(Is, Ip)
    # reconstruct_batch: faiss's decode, NaN for an absent id
    want = np.array([ids[7], ids[0], 5, ids[N - 1]], dtype=np.int64)
    rec = one.reconstruct_batch(want)
    assert np.isnan(rec[2]).all() and _same(rec[[0, 1, 3]], ref.decode(C[[7, 0, N - 1]], vmin, vdiff))
    assert np.abs(rec[0] - X[7]).max() <= vdiff.max() / 510 * 1.001      # within half a bin of what was added
    # remove_ids: byte for byte the index that received only the kept rows
    gone = np.sort(rng.permutation(N)[:777])
    keep = np.setdiff1d(np.arange(N), gone)
    assert staged.remove_ids(ids[gone]) == 777 and staged.remove_ids(ids[gone]) == 0
    fresh = FlatSQ8IPIndex(d)
    fresh.set_trained(vmin, vdiff)
    fresh.add_with_ids(X[keep], ids[keep])
    Cr, ir = staged.rows_host()
    Cf, if_ = fresh.rows_host()
    assert Cr.tobytes() == Cf.tobytes() == C[keep].tobytes() and np.array_equal(ir, if_) and staged.ntotal == N - 777
    assert staged.hbm_bytes() == (N - 777) * (d + 8) + 8 * d
    D1, I1 = staged.search(Q, 20)
    D2, I2 = fresh.search(Q, 20)
    D3, I3 = ref.topk(S[:, keep], 20, ids=ids[keep])
    assert _same(D1, D2) and _same(I1, I2) and _same(D1, D3) and _same(I1, I3)
    staged.add_with_ids(X[gone[:50]], ids[gone[:50]])                    # the reserved tensor is filled from the new end
    assert staged.ntotal == N - 727 and staged.rows_host()[0].tobytes() == np.concatenate([C[keep], C[gone[:50]]]).tobytes()
    assert one.remove_ids(IDSelectorRange(0, 10 ** 9)) == N and one.ntotal == 0
    D, I = one.search(Q, 3)
    assert (I == -1).all() and (D == NEG).all()


def test_index_class_routes_batches_to_the_matrix_cores():
    from wise_amd.index.flat_sq import FlatSQ8IPIndex

    N, d = 12000, 512
    C, T, Q = clustered_codes(N, d, 29)
    idx = FlatSQ8IPIndex(d)
    idx.set_trained(T[:d], T[d:])
    idx.adopt(C, _dev(np.arange(N, dtype=np.int64) * 2))
    assert FlatSQ8IPIndex.BATCH_MIN_ROWS == 1 << 18 and FlatSQ8IPIndex.BATCH_MIN_QUERIES == 8      # provisional: the sibling's floors
    De, Ie = idx.search_device(Q[:40], 10)                               # under the floor: the exact scan
    assert idx.batched_counts() == (0, 0)
    idx.BATCH_MIN_ROWS = 4096
    D, I = idx.search_device(Q[:40], 10)
    assert idx.batched_counts() == (40, 0) and _same(D, De) and _same(I, Ie)
    D2, I2 = idx.search_device(Q[:2], 10)                                # two queries: no batched shape
    assert sum(idx.batched_counts()) == 40 and _same(D2, De[:2]) and _same(I2, Ie[:2])
    D7, I7 = idx.search_device(Q[:7], 10)                                # under the query floor: the exact scan's passes
    assert sum(idx.batched_counts()) == 40 and _same(D7, De[:7]) and _same(I7, Ie[:7])
    D8, I8 = idx.search_device(Q[:8], 10)
    assert sum(idx.batched_counts()) == 48 and _same(D8, De[:8]) and _same(I8, Ie[:8])
    D3, I3 = idx.search_device(Q[:40], 200)                              # k > 128: the exact scan
    assert sum(idx.batched_counts()) == 48 and _same(I3[:, :10], Ie)


# ------------------------------------------------------------------------------------------------------------------ (7) files, sharding
def test_file_digest_after_create_load_and_update_through_the_plugin(tmp_path):
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    from wise_amd.index import faiss_io
    from wise_amd.index.flat_sq import FlatSQ8IPIndex
    from wise_amd.index.search_index_factory import SearchIndexFactory

    def write_store(X, ids):
        import shutil
        shutil.rmtree(tmp_path / "features", ignore_errors=True)
        (tmp_path / "features").mkdir()
        st = FeatureStoreFactory.create_store(FeatureStoreType.NUMPY, "video", str(tmp_path / "features"))
        st.enable_write(500, 0)
        for i, v in zip(ids, X):
            st.add(int(i), v[None])
        st.close()

    def digest(trained, C, ids):
        fn = tmp_path / "want.faiss"
        faiss_io.write_idmap_sq8_ip(fn, trained, C, ids)
        return hashlib.sha256(fn.read_bytes()).hexdigest()

    N, d = 1500, 64
    rng = np.random.default_rng(31)
    X = rng.standard_normal((N, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    ids = np.arange(N, dtype=np.int64) * 2 + 1
    write_store(X, ids)
    si = SearchIndexFactory("video", "mlfoundations/open_clip/ViT-B-32/seeded-0", {"features_dir": tmp_path / "features", "index_dir": tmp_path / "index"})
    itype = "IndexSQ8bit"
    si.create_index(itype)
    fn = si.get_index_filename(itype)
    vmin, vdiff = ref.train(X)                                           # over EVERY row of the store
    C = ref.encode(X, vmin, vdiff)
    trained = np.concatenate([vmin, vdiff])
    assert hashlib.sha256(fn.read_bytes()).hexdigest() == digest(trained, C, ids)
    assert C.min() == 0 and C.max() >= 254 and faiss_io.flat_sq_qtype(fn) == 0      # trained over every row: the ranges are used up
    idx = si._index_from_file(fn)
    assert type(idx) is FlatSQ8IPIndex and idx.ntotal == N and idx.rows_host()[0].tobytes() == C.tobytes()
    Q = rng.standard_normal((3, d)).astype(np.float32)
    S = ref.scores(C, vmin, vdiff, Q)
    D, I = idx.search(Q, 10)
    Dr, Ir = ref.topk(S, 10, ids=ids)
    assert _same(D, Dr) and _same(I, Ir)
    # update_index: 100 vectors leave, 60 arrive (some outside the ranges as trained: they clamp); the ranges stay
    gone = np.sort(rng.permutation(N)[:100])
    stay = np.setdiff1d(np.arange(N), gone)
    newX = (rng.standard_normal((60, d)) * 0.3).astype(np.float32)
    new_ids = np.arange(60, dtype=np.int64) + 10 ** 6
    write_store(np.concatenate([X[stay], newX]), np.concatenate([ids[stay], new_ids]))
    assert si.update_index(itype) == (60, 100)
    C2 = np.concatenate([C[stay], ref.encode(newX, vmin, vdiff)])
    assert hashlib.sha256(fn.read_bytes()).hexdigest() == digest(trained, C2, np.concatenate([ids[stay], new_ids]))
    assert si.update_index(itype) == (0, 0)


@pytest.mark.parametrize("W", [1, 3, 8])
def test_slices_merged_in_rank_order_are_the_whole_index(W):
    N, d, nq = 6001, 48, 4
    C, vmin, vdiff, X, dup = make_rows(N, d, 61)
    for r in range(1, W):                                                # equal rows on both sides of every slice boundary
        lo = shard_range(N, r, W)[0]
        C[lo], X[lo] = C[lo - 1], X[lo - 1]
        dup.append(lo - 1)
    Q = make_queries(X, dup[-3:], nq, 12)
    S = ref.scores(C, vmin, vdiff, Q)
    ids = np.random.default_rng(7).permutation(N).astype(np.int64) + 1
    whole = _index(d, C, vmin, vdiff, ids)
    for k in (1, 10, 100):
        De, Ie = whole.search_device(_dev(Q), k)
        Dr, Ir = ref.topk(S, k, ids=ids)
        assert _same(De, Dr) and _same(Ie, Ir)
        Ds, Is = [], []
        for r in range(W):
            lo, hi = shard_range(N, r, W)
            D, I = _index(d, C[lo:hi], vmin, vdiff, ids[lo:hi]).search_device(_dev(Q), k)
            Ds.append(D)
            Is.append(I)
        D, I = merge_device(torch.stack(Ds), torch.stack(Is), k)
        assert _same(D, De) and _same(I, Ie), (W, k)


def test_sharded_plugin_over_rccl_world1(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "sharded_sq8_nccl_worker.py"), str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert res["ok"], json.dumps(res)
    assert res["exchange_bytes"] == 16 * 3 * 10                          # one exchange of (score, id) planes: nq = 3, k = 10

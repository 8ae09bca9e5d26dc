"""-m gpu: IndexSQfp16 (csrc/ip_sq16.hip, wise_amd/index/flat_sq.py) — every path bit for bit against tests/sqfp16_flat_ref.py, or,
for the batched search, against wise_ipsq16_topk on the same data.

(1) the exact scan over shapes that take every path of it (rows per wave-load 64 .. 1, 1 / 2 / 4 queries a pass, list lengths,
    several blocks and a ragged tail), with subnormal halves, signed zeros and duplicate rows across a block boundary;
(2) the scan over a list of positions; (3) range count / fill through range_search.run; (4) the batched search, its constructed
    overflow and its refusals; (5) graph capture; (6) the index class; (7) slices merged in rank order, and the plugin on RCCL."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import sqfp16_flat_ref as ref
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
    """halves [N,d] float16 with what the contract must carry through: subnormals, signed zeros, a duplicate pair on both sides of
    a block boundary and one at the two ends.  Returns (halves, rows whose copies exist)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, d)).astype(np.float32) / np.float32(np.sqrt(d))
    H = ref.encode(X)
    dup = []
    if N:
        r = rng.integers(0, N, size=max(N // 7, 1))
        H[r, rng.integers(0, d, size=r.size)] = np.float16(3e-7) * rng.choice([-1, 1], size=r.size).astype(np.float16)   # subnormal
        H[r, rng.integers(0, d, size=r.size)] = np.float16(-0.0)
        H[r[::2], rng.integers(0, d, size=r[::2].size)] = np.float16(0.0)
        H[0] = np.float16(2.0 ** -20)                                    # a row of subnormals only
    B = block_rows(d)
    if N > B + 1:
        H[B - 1] *= np.float16(4.0)                                      # long rows: under their own direction no other row comes near
        H[B] = H[B - 1]
        dup.append(B - 1)
    if N > 2:
        H[1] *= np.float16(4.0)
        H[N - 1] = H[1]
        dup.append(1)
    return H, dup


def make_queries(H, dup, nq, seed):
    d = H.shape[1]
    Q = np.random.default_rng(seed).standard_normal((nq, d)).astype(np.float32)
    for i, r in enumerate(dup[:nq]):
        Q[i] = H[r].astype(np.float32) * np.float32(3.0)                 # its copies share the best score
    return Q


def gpu_topk(Hd, N, d, Qd, k, ids=None, id_base=0, pos=None, fill=None):
    lib = _lib.lib()
    nq = Qd.shape[0]
    D = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    I = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    n_items = N if pos is None else pos.numel()
    need = lib.wise_ipsqfp16_topk_workspace_bytes(n_items, d, nq, k)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    if pos is None:
        rc = lib.wise_ipsq16_topk(_lib.ptr(Hd), N, d, Qd.data_ptr(), nq, k, _lib.ptr(ids), id_base, D.data_ptr(), I.data_ptr(),
                                  ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    else:
        rc = lib.wise_ipsq16_topk_pos(_lib.ptr(Hd), N, d, _lib.ptr(pos), pos.numel(), Qd.data_ptr(), nq, k, _lib.ptr(ids), id_base,
                                      D.data_ptr(), I.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "wise_ipsq16_topk")
    return D, I


# ------------------------------------------------------------------------------------------------------------------ (1) exact scan
@pytest.mark.parametrize("d", [16, 48, 512, 1024])
@pytest.mark.parametrize("N", [0, 1, 63, 6000])
def test_exact_scan_bit_for_bit(d, N):
    H, dup = make_rows(N, d, 100 + d + N)
    Q = make_queries(H, dup, 5, 7)
    S = ref.scores(H, Q)                                                 # once per shape, shared by every case below
    ids = np.random.default_rng(1).permutation(N).astype(np.int64) * 3 + 11
    Hd, Qd, idd = _dev(H.view(np.int16)).reshape(N, d), _dev(Q), _dev(ids)
    if N > block_rows(d) + 1:                                            # the duplicates: equal scores, the lower position first
        D, I = gpu_topk(Hd, N, d, Qd[:1], 10)
        I = I.cpu().numpy()[0]
        at = list(I).index(block_rows(d) - 1)
        assert I[at + 1] == block_rows(d) and _bits(D)[0, at] == _bits(D)[0, at + 1]
    for nq in (1, 4, 5):
        for k in (1, 10, 100, 1024):
            Dr, Ir = ref.topk(H, Q[:nq], k, S=S[:nq], id_base=5)
            D, I = gpu_topk(Hd, N, d, Qd[:nq], k, id_base=5)
            assert _same(D, Dr) and _same(I, Ir), (d, N, nq, k, "positions")
            Dr, Ir = ref.topk(H, Q[:nq], k, ids=ids, S=S[:nq])
            D, I = gpu_topk(Hd, N, d, Qd[:nq], k, ids=idd)
            assert _same(D, Dr) and _same(I, Ir), (d, N, nq, k, "ids")
            if N < k:                                                    # padding
                assert (Ir[:, N:] == -1).all() and (Dr[:, N:] == NEG).all()


def test_exact_scan_several_blocks_and_a_ragged_tail():
    d, N = 16, 70001
    assert N > 4 * block_rows(d) and N % (64 // (d // 16)) != 0
    H, dup = make_rows(N, d, 5)
    Q = make_queries(H, dup, 5, 8)
    S = ref.scores(H, Q)
    Hd, Qd = _dev(H.view(np.int16)), _dev(Q)
    for nq, k in ((1, 10), (5, 100), (4, 1024), (2, 2048)):
        Dr, Ir = ref.topk(H, Q[:nq], k, S=S[:nq])
        D, I = gpu_topk(Hd, N, d, Qd[:nq], k)
        assert _same(D, Dr) and _same(I, Ir), (nq, k)
    I = gpu_topk(Hd, N, d, Qd[:2], 10)[1].cpu().numpy()
    assert list(I[0]).index(block_rows(d) - 1) + 1 == list(I[0]).index(block_rows(d))      # across a block boundary
    assert list(I[1]).index(1) + 1 == list(I[1]).index(N - 1)                             # across the whole grid


# ------------------------------------------------------------------------------------------------------------------ (2) positions
@pytest.mark.parametrize("d", [48, 512])
def test_position_scan_equals_the_restatement_restricted(d):
    N = 6000
    H, dup = make_rows(N, d, 31 + d)
    Q = make_queries(H, dup, 5, 9)
    S = ref.scores(H, Q)
    ids = np.arange(N, dtype=np.int64) * 2 + 1
    Hd, Qd, idd = _dev(H.view(np.int16)), _dev(Q), _dev(ids)
    rng = np.random.default_rng(2)
    sets = {"empty": np.zeros(0, np.int64), "one": np.array([block_rows(d)], np.int64), "every": np.arange(N, dtype=np.int64),
            "sparse": np.sort(rng.permutation(N)[:137]).astype(np.int64),
            "dups": np.array([1, block_rows(d) - 1, block_rows(d), N - 1], np.int64)}
    for name, pos in sets.items():
        pd = _dev(pos) if pos.size else torch.zeros(0, dtype=torch.int64, device="cuda")
        for nq in (1, 5):
            for k in (1, 10, 100):
                Dr, Ir = ref.topk_pos(H, Q[:nq], k, pos, ids=ids, S=S[:nq])
                D, I = gpu_topk(Hd, N, d, Qd[:nq], k, ids=idd, pos=pd)
                assert _same(D, Dr) and _same(I, Ir), (name, nq, k)
                if name == "every":
                    Da, Ia = gpu_topk(Hd, N, d, Qd[:nq], k, ids=idd)
                    assert _same(D, Da) and _same(I, Ia)
        Dr, Ir = ref.topk_pos(H, Q[:2], 10, pos, S=S[:2], id_base=3)
        D, I = gpu_topk(Hd, N, d, Qd[:2], 10, id_base=3, pos=pd)
        assert _same(D, Dr) and _same(I, Ir), name


# ------------------------------------------------------------------------------------------------------------------ (3) range
@pytest.mark.parametrize("d", [16, 512])
def test_range_search_is_the_prefix_of_the_exact_scan(d):
    from wise_amd.index.flat_sq import FlatSQfp16IPIndex
    from wise_amd.index.selector import IDSelectorBatch

    N, nq = 6000, 5
    H, dup = make_rows(N, d, 41 + d)
    Q = make_queries(H, dup, nq, 10)
    S = ref.scores(H, Q)
    ids = np.random.default_rng(3).permutation(N).astype(np.int64) + 100
    idx = FlatSQfp16IPIndex(d).adopt(_dev(H.view(np.int16)), _dev(ids))
    D2k, I2k = gpu_topk(idx._H, N, d, _dev(Q), 2048, ids=idx._ids)
    D2k, I2k = D2k.cpu().numpy(), I2k.cpu().numpy()
    chosen = np.sort(np.random.default_rng(4).permutation(ids)[:N // 3])
    keep = np.isin(ids, chosen)
    kth = np.sort(S, axis=1)
    for thr in (float(kth[:, -40].max()), float(kth[:, -1500].min()), float(S.max()), float(NEG)):    # a few, many, none, every row
        for sel, mask in ((None, None), (IDSelectorBatch(chosen), keep)):
            lims, D, I = (t.cpu().numpy() for t in idx.range_search_device(_dev(Q), thr, sel=sel, chunk=2))
            lr, Dr, Ir = ref.range_search(H, Q, thr, ids=ids, keep=mask, S=S)
            assert np.array_equal(lims, lr) and _same(D, Dr) and _same(I, Ir), (d, thr, sel is not None)
            if mask is None:                                             # the check of tests/test_gpu_range.py: a prefix of the top-2048
                for q in range(nq):
                    n = min(int(lims[q + 1] - lims[q]), 2048)
                    assert _same(D[lims[q]:lims[q] + n], D2k[q, :n]) and _same(I[lims[q]:lims[q] + n], I2k[q, :n])
    lims, D, I = idx.range_search(Q, float(S.max()))
    assert lims.tolist() == [0] * (nq + 1) and D.size == 0 and I.size == 0
    lims, _, _ = idx.range_search(Q[:1], float(NEG))
    assert lims.tolist() == [0, N]
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            idx.range_search(Q, bad)


# ------------------------------------------------------------------------------------------------------------------ (4) batched
def gpu_batched(Hd, norms, N, d, Qd, k, ids=None, id_base=0, counters=None):
    lib = _lib.lib()
    nq = Qd.shape[0]
    D = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    I = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    need = lib.wise_ipsqfp16_topk_batched_workspace_bytes(N, d, nq, k)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _lib.check(lib.wise_ipsq16_topk_batched(Hd.data_ptr(), norms.data_ptr(), N, d, Qd.data_ptr(), nq, k, _lib.ptr(ids), id_base,
                                            D.data_ptr(), I.data_ptr(), _lib.ptr(counters), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               "wise_ipsq16_topk_batched")
    return D, I


def prepare(Hd, N, d):
    norms = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().wise_ipsq16_prepare(Hd.data_ptr(), N, d, norms.data_ptr(), _lib.stream_ptr()), "wise_ipsq16_prepare")
    return norms


def clustered_halves(N, d, seed, scale=1.0):
    """unit rows around 64 centres (near neighbours: many scores close to a query's k-th), as halves on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    c = torch.randn(64, d, device="cuda", generator=g)
    c /= c.norm(dim=1, keepdim=True)
    e = torch.randn(N, d, device="cuda", generator=g)
    X = c[torch.randint(0, 64, (N,), device="cuda", generator=g)] + 0.35 * e / e.norm(dim=1, keepdim=True)
    X = X / X.norm(dim=1, keepdim=True) * scale
    Q = X[:130] + 0.05 * torch.randn(130, d, device="cuda", generator=g) / (d ** 0.5) * scale
    return X.to(torch.float16).contiguous(), Q.float().contiguous()


@pytest.mark.parametrize("d", [256, 512, 768, 1024])
def test_batched_search_has_the_bits_of_the_exact_scan(d):
    N = 40000
    Hd, Q = clustered_halves(N, d, 50 + d)
    Hd[30001] = Hd[17]                                                   # equal rows far apart
    norms = prepare(Hd, N, d)
    want = float(Hd.float().norm(dim=1).max())
    assert abs(float(norms[0]) - want) <= 1e-5 * want and _same(prepare(Hd, N, d), norms)      # deterministic
    ids = _dev(np.random.default_rng(6).permutation(N).astype(np.int64) + 9)
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    asked = 0
    for nq in (3, 64, 130):
        for k in (10, 100):
            De, Ie = gpu_topk(Hd, N, d, Q[:nq], k, ids=ids)
            D, I = gpu_batched(Hd, norms, N, d, Q[:nq], k, ids=ids, counters=counters)
            assert _same(D, De) and _same(I, Ie), (d, nq, k)
            asked += nq
    De, Ie = gpu_topk(Hd, N, d, Q[:7], 128, id_base=4)
    D, I = gpu_batched(Hd, norms, N, d, Q[:7], 128, id_base=4)          # no ids, no counters, the largest k
    assert _same(D, De) and _same(I, Ie)
    c = counters.cpu().numpy()
    assert int(c.sum()) == asked and int(c[0]) > 0, c                    # every query is counted once; the lists answered


def test_batched_search_with_subnormal_rows_and_large_queries():
    """Rows scaled into the binary16 subnormal range (every stored component below 2^-14) and queries scaled up: the matrix cores
    must take subnormal operands as they are, or the candidate scores leave the band."""
    N, d = 8192, 256
    Hd, Q = clustered_halves(N, d, 77, scale=2.0 ** -13)
    assert float(Hd.float().abs().max()) < 2.0 ** -13 and float((Hd.float().abs() < 2.0 ** -14).float().mean()) > 0.9
    Q = Q * 2.0 ** 20
    norms = prepare(Hd, N, d)
    for nq, k in ((5, 10), (40, 100)):
        De, Ie = gpu_topk(Hd, N, d, Q[:nq], k)
        D, I = gpu_batched(Hd, norms, N, d, Q[:nq], k)
        assert _same(D, De) and _same(I, Ie), (nq, k)


def test_batched_overflow_is_redone_by_the_exact_scan():
    N, d, k = 40000, 256, 10
    Hd, Q = clustered_halves(N, d, 91)
    q = torch.randn(d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(92))
    Q[3] = q / q.norm()                                                  # a direction of its own: no other query sees its copies
    q = Q[3].clone()
    h = q.to(torch.float16)
    copies = 6000                                                        # more than a candidate list holds (4096)
    where = torch.arange(copies, device="cuda") * 6 + 5                  # spread over the whole index
    rows = h.repeat(copies, 1)
    last = rows[:, d - 1].view(torch.int16)
    last ^= (torch.arange(copies, device="cuda") & 1).to(torch.int16)    # they differ in their last stored bit
    Hd[where] = rows
    norms = prepare(Hd, N, d)
    nq = 5
    De, Ie = gpu_topk(Hd, N, d, Q[:nq], k)
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    D, I = gpu_batched(Hd, norms, N, d, Q[:nq], k, counters=counters)
    assert _same(D, De) and _same(I, Ie)
    c = counters.cpu().numpy()
    assert c[1] > 0 and int(c.sum()) == nq, c                            # the fallback ran, every query counted once
    assert set(Ie[3].tolist()) <= set(where.tolist())                    # the copies are that query's answer
    # a pass without that query is answered from the lists
    counters.zero_()
    D, I = gpu_batched(Hd, norms, N, d, Q[:3], k, counters=counters)
    assert _same(D, De[:3]) and _same(I, Ie[:3]) and counters.cpu().numpy().tolist() == [3, 0]


@pytest.mark.parametrize("N", [6000, 40000])
def test_batched_query_beyond_the_range_of_binary16_takes_the_exact_scan(N):
    """A finite fp32 query with a component above 65504 has no binary16 image: its matrix-core scores would be inf, or NaN where a
    row holds a zero there (inf * 0) or where two such components meet with opposite signs (inf - inf).  The pass must be answered
    by the exact scan, whose fp32 scores of the same inputs are ordinary numbers."""
    d, k = 256, 10
    Hd, Q = clustered_halves(N, d, 33)
    Hd[:, 7] = 0.0                                                       # every row holds a zero at component 7
    Hd[::2, 7] = -0.0
    assert float((Hd[:, 3].float() * Hd[:, 9].float() > 0).float().mean()) > 0.3      # components 3 and 9: both sign patterns occur
    assert float((Hd[:, 3].float() * Hd[:, 9].float() < 0).float().mean()) > 0.3
    norms = prepare(Hd, N, d)
    Q = Q[:6].clone()
    Q[1, 7] = 1.0e5                                                      # against the zeros: inf * 0
    Q[2, 3], Q[2, 9] = 1.0e5, 1.2e5                                      # +inf and -inf on the rows of mixed sign
    Q[4, 200] = -7.0e4                                                   # one component just beyond the range
    assert bool(torch.isfinite(Q).all()) and not bool(torch.isfinite(Q.to(torch.float16)).all())
    De, Ie = gpu_topk(Hd, N, d, Q, k)
    assert bool(torch.isfinite(De).all()) and bool((Ie >= 0).all())
    for rows in ([0, 1, 3], [0, 2, 3, 5], [3, 4, 5], [0, 1, 2, 3, 4, 5]):
        counters = torch.zeros(2, dtype=torch.int32, device="cuda")
        q = Q[rows].contiguous()
        D, I = gpu_batched(Hd, norms, N, d, q, k, counters=counters)
        assert _same(D, De[rows]) and _same(I, Ie[rows]), rows
        assert counters.cpu().numpy().tolist() == [0, len(rows)], rows  # the exact scan answered the pass
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    D, I = gpu_batched(Hd, norms, N, d, Q[[0, 3, 5]].contiguous(), k, counters=counters)
    assert _same(D, De[[0, 3, 5]]) and _same(I, Ie[[0, 3, 5]]) and counters.cpu().numpy().tolist() == [3, 0]   # and without them, the lists


def test_batched_refusals_leave_the_outputs_untouched():
    lib = _lib.lib()
    N, d, nq, k = 4096, 256, 4, 10
    Hd, Q = clustered_halves(N, d, 13)
    Q = Q[:nq].contiguous()
    norms = prepare(Hd, N, d)
    for shape in ((N, 20, nq, k), (N, 128, nq, k), (N, 320, nq, k), (N, d, 2, k), (N, d, nq, 129), (N - 1, d, nq, k)):
        assert lib.wise_ipsqfp16_topk_batched_workspace_bytes(*shape) == 0, shape
    need = lib.wise_ipsqfp16_topk_batched_workspace_bytes(N, d, nq, k)
    ws = torch.empty(need + 64, dtype=torch.uint8, device="cuda")
    D = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    I = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    st = _lib.stream_ptr()

    def call(rows=Hd.data_ptr(), dd=d, qp=Q.data_ptr(), wsp=ws.data_ptr(), wsn=need, n=N, nqq=nq, kk=k):
        return lib.wise_ipsq16_topk_batched(rows, norms.data_ptr(), n, dd, qp, nqq, kk, 0, 0, D.data_ptr(), I.data_ptr(), 0, wsp, wsn, st)

    bad = {"short workspace": call(wsn=need - 1), "no workspace": call(wsp=0), "misaligned rows": call(rows=Hd.data_ptr() + 2),
           "misaligned queries": call(qp=Q.data_ptr() + 4), "d = 20": call(dd=20), "nq = 2": call(nqq=2), "k = 129": call(kk=129),
           "N = 4095": call(n=N - 1)}
    torch.cuda.synchronize()
    assert all(rc == WISE_E_INVALID for rc in bad.values()), bad
    assert lib.wise_last_error()
    assert bool((D == 7.0).all()) and bool((I == 7).all())
    # the exact scan's own refusals
    wse = torch.empty(lib.wise_ipsqfp16_topk_workspace_bytes(N, d, nq, k), dtype=torch.uint8, device="cuda")
    for rc in (lib.wise_ipsq16_topk(Hd.data_ptr(), N, 20, Q.data_ptr(), nq, k, 0, 0, D.data_ptr(), I.data_ptr(), wse.data_ptr(), wse.numel(), st),
               lib.wise_ipsq16_topk(Hd.data_ptr() + 2, N, d, Q.data_ptr(), nq, k, 0, 0, D.data_ptr(), I.data_ptr(), wse.data_ptr(), wse.numel(), st),
               lib.wise_ipsq16_topk(Hd.data_ptr(), N, d, Q.data_ptr(), nq, k, 0, 0, D.data_ptr(), I.data_ptr(), wse.data_ptr(), wse.numel() - 512, st),
               lib.wise_ipsq16_topk(Hd.data_ptr(), N, d, Q.data_ptr(), nq, 2049, 0, 0, D.data_ptr(), I.data_ptr(), wse.data_ptr(), wse.numel(), st)):
        assert rc == WISE_E_INVALID
    torch.cuda.synchronize()
    assert bool((D == 7.0).all()) and bool((I == 7).all())
    assert call() == 0                                                   # and the good call goes through
    torch.cuda.synchronize()
    De, Ie = gpu_topk(Hd, N, d, Q, k)
    assert _same(D, De) and _same(I, Ie)


# ------------------------------------------------------------------------------------------------------------------ (5) graph capture
def test_graph_capture_of_the_exact_and_of_the_batched_search():
    lib = _lib.lib()
    N, d, nq, k = 8192, 256, 6, 10
    Hd, Q = clustered_halves(N, d, 17)
    Q = Q[:nq].contiguous()
    norms = prepare(Hd, N, d)
    De, Ie = gpu_topk(Hd, N, d, Q, k)
    Dw, Iw = gpu_batched(Hd, norms, N, d, Q, k)                          # both paths have run once before the capture
    assert _same(Dw, De) and _same(Iw, Ie)
    outs = [(torch.zeros(nq, k, dtype=torch.float32, device="cuda"), torch.zeros(nq, k, dtype=torch.int64, device="cuda")) for _ in range(2)]
    wse = torch.empty(lib.wise_ipsqfp16_topk_workspace_bytes(N, d, nq, k), dtype=torch.uint8, device="cuda")
    wsb = torch.empty(lib.wise_ipsqfp16_topk_batched_workspace_bytes(N, d, nq, k), dtype=torch.uint8, device="cuda")
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = _lib.stream_ptr()
        _lib.check(lib.wise_ipsq16_topk(Hd.data_ptr(), N, d, Q.data_ptr(), nq, k, 0, 0, outs[0][0].data_ptr(), outs[0][1].data_ptr(),
                                        wse.data_ptr(), wse.numel(), st))
        _lib.check(lib.wise_ipsq16_topk_batched(Hd.data_ptr(), norms.data_ptr(), N, d, Q.data_ptr(), nq, k, 0, 0, outs[1][0].data_ptr(),
                                                outs[1][1].data_ptr(), counters.data_ptr(), wsb.data_ptr(), wsb.numel(), st))
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
    from wise_amd.index.flat_sq import FlatSQfp16IPIndex
    from wise_amd.index.selector import IDSelectorRange, SearchParameters

    N, d = 5000, 48
    rng = np.random.default_rng(23)
    X = (rng.standard_normal((N, d)) / np.sqrt(d)).astype(np.float32)
    X[7, :5] = np.array([1e-7, -1e-7, 0.0, -0.0, 6.1e-5], dtype=np.float32)      # subnormals, signed zeros, the edge of the normals
    ids = rng.permutation(N).astype(np.int64) + 1000
    H = ref.encode(X)
    one = FlatSQfp16IPIndex(d)
    one.add_with_ids(X, ids)
    chunked = FlatSQfp16IPIndex(d)
    chunked.ENCODE_BYTES = 4 * d * 300                                   # the encoder's own staging: 300 rows at a time
    for s in range(0, N, 1234):
        chunked.add_with_ids(X[s:s + 1234], ids[s:s + 1234])
    reserved = FlatSQfp16IPIndex(d)
    reserved.reserve(N)
    for s in range(0, N, 2000):
        reserved.add_with_ids(_dev(X[s:s + 2000]), ids[s:s + 2000])      # rows already on the device
    adopted = FlatSQfp16IPIndex(d).adopt(_dev(H.view(np.int16)).view(torch.float16), _dev(ids))
    loaded = FlatSQfp16IPIndex(d)
    loaded.reserve(N)
    loaded.add_halves_with_ids(H[:3000], ids[:3000])
    loaded.add_halves_with_ids(H[3000:], ids[3000:])
    Q = rng.standard_normal((5, d)).astype(np.float32)
    Dr, Ir = ref.topk(H, Q, 20, ids=ids)
    for idx in (one, chunked, reserved, adopted, loaded):
        Hh, ih = idx.rows_host()
        assert Hh.tobytes() == H.tobytes() and np.array_equal(ih, ids)   # numpy's cast, whatever the chunking
        assert idx.ntotal == N and idx.is_trained and idx.hbm_bytes() == N * (2 * d + 8)
        assert idx._H.dtype == torch.float16 and not hasattr(idx, "_X")  # no fp32 rows, no shadow
        D, I = idx.search(Q, 20)
        assert _same(D, Dr) and _same(I, Ir)
    # a selector: the scan over the selected positions
    sel = IDSelectorRange(1500, 2500)
    pos = np.flatnonzero((ids >= 1500) & (ids < 2500))
    Ds, Is = one.search(Q, 20, params=SearchParameters(sel=sel))
    Dp, Ip = ref.topk_pos(H, Q, 20, pos, ids=ids)
    assert _same(Ds, Dp) and _same(Is, Ip)
    # reconstruct_batch: float32(float16(x)), NaN for an absent id
    want = np.array([ids[7], ids[0], 5, ids[N - 1]], dtype=np.int64)
    rec = one.reconstruct_batch(want)
    assert np.isnan(rec[2]).all() and _same(rec[[0, 1, 3]], H[[7, 0, N - 1]].astype(np.float32))
    assert rec[0, 0] != 0 and np.signbit(rec[0, 3])
    # the encoder at the edges of binary16, away from any search: overflow to inf, ties to even, the smallest subnormal
    edge = np.zeros((3, 16), dtype=np.float32)
    edge[0, :8] = [65504.0, 65519.9, 65520.0, -70000.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001, 1.0 + 2.0 ** -11]
    edge[1, :4] = [1.0 + 3 * 2.0 ** -11, -(2.0 ** -14), 2.0 ** -14 - 2.0 ** -26, np.float32(1e-8)]
    tiny = FlatSQfp16IPIndex(16)
    tiny.add_with_ids(edge, np.arange(3))
    assert tiny.rows_host()[0].tobytes() == ref.encode(edge).tobytes() and np.isinf(tiny.rows_host()[0][0, 2:4].astype(np.float32)).all()
    # remove_ids: byte for byte the index that received only the kept rows
    gone = np.sort(rng.permutation(N)[:777])
    keep = np.setdiff1d(np.arange(N), gone)
    assert reserved.remove_ids(ids[gone]) == 777 and reserved.remove_ids(ids[gone]) == 0
    fresh = FlatSQfp16IPIndex(d)
    fresh.add_with_ids(X[keep], ids[keep])
    Hr, ir = reserved.rows_host()
    Hf, if_ = fresh.rows_host()
    assert Hr.tobytes() == Hf.tobytes() == H[keep].tobytes() and np.array_equal(ir, if_) and reserved.ntotal == N - 777
    assert reserved.hbm_bytes() == (N - 777) * (2 * d + 8)
    D1, I1 = reserved.search(Q, 20)
    D2, I2 = fresh.search(Q, 20)
    D3, I3 = ref.topk(H[keep], Q, 20, ids=ids[keep])
    assert _same(D1, D2) and _same(I1, I2) and _same(D1, D3) and _same(I1, I3)
    assert _same(reserved.search(Q, 20, params=SearchParameters(sel=sel))[1], fresh.search(Q, 20, params=SearchParameters(sel=sel))[1])
    reserved.add_with_ids(X[gone[:50]], ids[gone[:50]])                  # the reserved tensor is filled from the new end
    assert reserved.ntotal == N - 727 and reserved.rows_host()[0].tobytes() == np.concatenate([H[keep], H[gone[:50]]]).tobytes()
    assert one.remove_ids(IDSelectorRange(0, 10 ** 9)) == N and one.ntotal == 0
    D, I = one.search(Q, 3)
    assert (I == -1).all() and (D == NEG).all()


def test_index_class_routes_batches_to_the_matrix_cores():
    from wise_amd.index.flat_sq import FlatSQfp16IPIndex

    N, d = 12000, 512
    Hd, Q = clustered_halves(N, d, 29)
    ids = _dev(np.arange(N, dtype=np.int64) * 2)
    idx = FlatSQfp16IPIndex(d).adopt(Hd, ids)
    assert FlatSQfp16IPIndex.BATCH_MIN_ROWS == 1 << 18                   # the provisional floor: FlatIPIndex's
    De, Ie = idx.search_device(Q[:40], 10)                               # under the floor: the exact scan
    assert idx.batched_counts() == (0, 0)
    idx.BATCH_MIN_ROWS = 4096
    D, I = idx.search_device(Q[:40], 10)
    assert sum(idx.batched_counts()) == 40 and _same(D, De) and _same(I, Ie)
    D2, I2 = idx.search_device(Q[:2], 10)                                # two queries: no batched shape
    assert sum(idx.batched_counts()) == 40 and _same(D2, De[:2]) and _same(I2, Ie[:2])
    assert FlatSQfp16IPIndex.BATCH_MIN_QUERIES == 8                      # under the measured crossover: the exact scan's passes
    D7, I7 = idx.search_device(Q[:7], 10)
    assert sum(idx.batched_counts()) == 40 and _same(D7, De[:7]) and _same(I7, Ie[:7])
    D8, I8 = idx.search_device(Q[:8], 10)
    assert sum(idx.batched_counts()) == 48 and _same(D8, De[:8]) and _same(I8, Ie[:8])
    D3, I3 = idx.search_device(Q[:40], 200)                              # k > 128: the exact scan
    assert sum(idx.batched_counts()) == 48 and _same(I3[:, :10], Ie)


# ------------------------------------------------------------------------------------------------------------------ (7) sharding
@pytest.mark.parametrize("W", [1, 3, 8])
def test_slices_merged_in_rank_order_are_the_whole_index(W):
    from wise_amd.index.flat_sq import FlatSQfp16IPIndex

    N, d, nq = 6001, 48, 4
    H, dup = make_rows(N, d, 61)
    for r in range(1, W):                                                # equal rows on both sides of every slice boundary
        lo = shard_range(N, r, W)[0]
        H[lo] = H[lo - 1]
        dup.append(lo - 1)
    Q = make_queries(H, dup[-3:], nq, 12)
    ids = np.random.default_rng(7).permutation(N).astype(np.int64) + 1
    whole = FlatSQfp16IPIndex(d).adopt(_dev(H.view(np.int16)), _dev(ids))
    for k in (1, 10, 100):
        De, Ie = whole.search_device(_dev(Q), k)
        Dr, Ir = ref.topk(H, Q, k, ids=ids)
        assert _same(De, Dr) and _same(Ie, Ir)
        Ds, Is = [], []
        for r in range(W):
            lo, hi = shard_range(N, r, W)
            part = FlatSQfp16IPIndex(d).adopt(_dev(H[lo:hi].view(np.int16)), _dev(ids[lo:hi]))
            D, I = part.search_device(_dev(Q), k)
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
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "sharded_sqfp16_nccl_worker.py"), str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert res["ok"], json.dumps(res)
    assert res["exchange_bytes"] == 16 * 3 * 10                          # one exchange of (score, id) planes: nq = 3, k = 10

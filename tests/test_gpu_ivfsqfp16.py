"""-m gpu: IndexIVFSQfp16 — wise_sq16_* and wise_ivfsq16_scan(_sel), wise_ivfsq16_range_* through the C ABI against the numpy
restatement (tests/ivfsqfp16_ref.py), bit for bit, then the index class, its selectors, range_search, remove_ids and the
SearchIndexFactory path on top of them."""
import os
import struct

import numpy as np
import pytest
import torch

import ivfsqfp16_ref as h16
import range_ref as rr
from wise_amd import _lib
from wise_amd.index import faiss_io
from wise_amd.index.ivf_flat import reference_nlist
from wise_amd.index.ivf_sq import IVFSQfp16IPIndex
from wise_amd.index.selector import IDSelectorBatch, IDSelectorNot, IDSelectorRange, SearchParametersIVF

pytestmark = pytest.mark.gpu

WISE_E_INVALID = -1
K = 2048


def unit_rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def hbits(a):
    return np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)


def gpu_encode(resid):
    n, d = resid.shape
    r_d = dev(resid)
    out = torch.empty(n, d, dtype=torch.float16, device="cuda")
    _lib.check(_lib.lib().wise_sq16_encode(r_d.data_ptr(), n, d, out.data_ptr(), _lib.stream_ptr()), "wise_sq16_encode")
    return out.cpu().numpy()


def gpu_decode(halves, pos, list_off, c):
    N, d = halves.shape
    a = [dev(x) for x in (halves, pos, list_off, c)]
    out = torch.empty(len(pos), d, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().wise_sq16_decode(a[0].data_ptr(), N, a[1].data_ptr(), len(pos), a[2].data_ptr(), len(c), a[3].data_ptr(), d,
                                           out.data_ptr(), _lib.stream_ptr()), "wise_sq16_decode")
    return out.cpu().numpy()


def gpu_bias(Q, c, probes):
    nq, nprobe = probes.shape
    Q_d, c_d, p_d = dev(Q), dev(c), dev(probes)
    bias = torch.empty(nq, nprobe, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().wise_pq_bias(Q_d.data_ptr(), c_d.data_ptr(), p_d.data_ptr(), nq, nprobe, c.shape[0], c.shape[1], bias.data_ptr(),
                                       _lib.stream_ptr()), "wise_pq_bias")
    return bias


def keep_words(keep):
    """bool [N] -> uint32 words, bit (p & 31) of word p >> 5 (what wise_sel_bitmap writes), as int32 for torch"""
    n = len(keep)
    padded = np.zeros((n + 31) // 32 * 32, dtype=np.uint8)
    padded[:n] = keep
    return np.packbits(padded, bitorder="little").view(np.int32)


class Case:
    """An index on the device: halves, list offsets, ids, centroids."""

    def __init__(self, halves, list_off, ids, c):
        self.halves, self.list_off, self.ids, self.c = halves, list_off, ids, c
        self.N, self.d = halves.shape
        self.nlist = len(list_off) - 1
        self.h_d, self.off_d, self.ids_d = dev(halves), dev(list_off), dev(ids)

    def raw_scan(self, Q_d, probes_d, bias_d, k, keep_d=None, ws_bytes=None, d=None, null=None):
        lib = _lib.lib()
        nq, nprobe = probes_d.shape
        need = lib.wise_ivfsq_scan_workspace_bytes(nq, nprobe, k)
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
        D = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
        I = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
        a = dict(h=self.h_d.data_ptr(), Q=Q_d.data_ptr(), probes=probes_d.data_ptr(), bias=bias_d.data_ptr(), D=D.data_ptr())
        if null is not None:
            a[null] = 0
        head = (a["h"], self.N, self.d if d is None else d, self.off_d.data_ptr(), self.nlist, self.ids_d.data_ptr(), a["Q"], nq, a["probes"],
                a["bias"], nprobe, k)
        tail = (a["D"], I.data_ptr(), ws.data_ptr(), need if ws_bytes is None else ws_bytes, _lib.stream_ptr())
        rc = lib.wise_ivfsq16_scan(*head, *tail) if keep_d is None else lib.wise_ivfsq16_scan_sel(*head, keep_d.data_ptr(), *tail)
        return rc, D, I

    def scan(self, Q_d, probes_d, bias_d, k, keep_d=None):
        rc, D, I = self.raw_scan(Q_d, probes_d, bias_d, k, keep_d)
        _lib.check(rc, "wise_ivfsq16_scan")
        return D.cpu().numpy(), I.cpu().numpy()


def lengths(d):
    """list lengths around the kernel's geometry: RPL = 64 / (d / 16) rows per wave-load, 4 waves x SQ_T = 4 loads per block pass"""
    rpl = 64 // (d // 16)
    return (0, 1, max(rpl - 1, 0), rpl + 1, 16 * rpl + 37, 40, 40, 2 * rpl)


def scan_case(d):
    """lists of lengths(d) rows of residual-like halves; rows of subnormal halves and of -0; equal rows twice within the long list
    and in the two lists of 40 rows, whose centroids are equal (equal bias: ties across lists); ids a permutation"""
    rng = np.random.default_rng(100 + d)
    L = lengths(d)
    list_off = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
    N = int(list_off[-1])
    halves = (rng.standard_normal((N, d)) * 0.1).astype(np.float32).astype(np.float16)
    lo = int(list_off[4])
    n_long = L[4]
    sub = (rng.integers(1, 0x400, (6, d)).astype(np.uint16) | (rng.integers(0, 2, (6, d)).astype(np.uint16) << 15)).view(np.float16)
    halves[lo + 3:lo + 9] = sub                                  # every element a subnormal half, either sign
    halves[lo + 9:lo + 11] = np.float16(-0.0)
    halves[lo + n_long - 5:lo + n_long - 2] = halves[lo + 12:lo + 15]   # equal rows within one list: the first in list order wins
    a, b = int(list_off[5]), int(list_off[6])
    halves[b:b + 40] = halves[a:a + 40]                          # and in two lists
    c = unit_rows(len(L), d, d + 1)
    c[6] = c[5]
    ids = rng.permutation(N).astype(np.int64) * 7 + 1
    return Case(halves, list_off, ids, c)


def probe_sets(nlist, nq):
    """nprobe -> [nq, nprobe]: 1 probe = the lists of 0 / 1 rows; more = rotations of the lists; nlist + 4 with -1, a value >= nlist
    and a list named twice"""
    out = {1: np.array([[0], [1], [4]], dtype=np.int64)[:nq]}
    rot = np.stack([np.roll(np.arange(nlist, dtype=np.int64)[::-1], q) for q in range(nq)])
    out[3] = rot[:, :3].copy()
    out[nlist] = rot.copy()
    wide = np.full((nq, nlist + 4), -1, dtype=np.int64)
    wide[:, [0, 2, 3, 5, 6, 7, 9, 10]] = rot
    wide[:, 4] = nlist + 2
    wide[:, 11] = rot[:, 1]                                       # the same list again
    out[nlist + 4] = wide
    return out


def prefix(Dfull, Ifull, k):
    nq, kf = Dfull.shape
    D = np.full((nq, k), h16.NEG, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    D[:, :min(k, kf)], I[:, :min(k, kf)] = Dfull[:, :k], Ifull[:, :k]
    return D, I


@pytest.mark.parametrize("d", [16, 48, 512])
def test_encode_and_decode_give_the_restatements_bits(d):
    rng = np.random.default_rng(d)
    n = 300
    resid = (rng.standard_normal((n, d)) * 0.1).astype(np.float32)
    f = np.float32
    special = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 0.1 + 0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25,
                        1.5 * 2.0 ** -24, 2.0 ** -15, -(2.0 ** -20), 2.0 ** -14 - 2.0 ** -25, 2.0 ** -26, -0.0, 0.0, 65504.0, 70000.0], dtype=f)
    assert d >= len(special)
    resid[0, :len(special)] = special
    # exact ties between two neighbouring halves, to an even and to an odd lower neighbour, over many exponents
    base = rng.integers(0x0400, 0x7800, d).astype(np.uint16)
    lo16 = base.view(np.float16).astype(np.float64)
    hi16 = (base + 1).astype(np.uint16).view(np.float16).astype(np.float64)
    resid[1] = ((lo16 + hi16) / 2).astype(f)                     # representable in float32: exactly half way
    assert ((base & 1) == 0).any() and ((base & 1) == 1).any()
    assert np.array_equal(resid[1].astype(np.float64), (lo16 + hi16) / 2)
    resid[2] = (rng.uniform(2.0 ** -24, 0.99 * 2.0 ** -14, d) * rng.choice([-1, 1], d)).astype(f)      # the subnormal range
    want = h16.encode(resid)
    got = gpu_encode(resid)
    assert np.array_equal(hbits(got), hbits(want)), d
    assert hbits(want)[0, 14] == 0x7BFF and hbits(want)[0, 15] == 0x7C00 and hbits(want)[0, 12] == 0x8000 and hbits(want)[0, 4] == 0x0001
    assert ((hbits(want)[2] & 0x7C00) == 0).all() and (hbits(want)[2] & 0x03FF).any()
    assert np.array_equal(hbits(want)[1], np.where(base & 1, base + 1, base))               # ties went to the even neighbour
    list_off = np.array([0, n // 3, n // 3, n], dtype=np.int64)     # three lists, the middle one empty
    c = unit_rows(3, d, d)
    pos = np.concatenate([np.arange(n), [-1, n, n + 5]]).astype(np.int64)
    finite = want.copy()
    finite[0, 15] = np.float16(1.0)                              # (inf + c is inf on both sides; keep the comparison about finite rows)
    dec = gpu_decode(finite, pos, list_off, c)
    assert np.array_equal(bits(dec[:n]), bits(h16.decode_rows(finite, list_off, c))), d
    assert np.isnan(dec[n:]).all()


@pytest.mark.parametrize("d", [16, 48, 512, 1024])
def test_scan_is_bit_equal_to_the_restatement(d):
    case = scan_case(d)
    Q3 = unit_rows(3, d, d + 9) * np.float32(1.3)
    for nq in (1, 3):
        Q = Q3[:nq]
        Q_d = dev(Q)
        for nprobe, probes in probe_sets(case.nlist, nq).items():
            bias_d = gpu_bias(Q, case.c, probes)
            bias = bias_d.cpu().numpy()
            Dfull, Ifull = h16.scan(case.halves, case.list_off, case.ids, Q, probes, bias, 100)
            for k in (1, 10, 100):
                D, I = case.scan(Q_d, dev(probes), bias_d, k)
                Do, Io = prefix(Dfull, Ifull, k)
                what = f"d={d} nq={nq} nprobe={nprobe} k={k}"
                assert np.array_equal(bits(D), bits(Do)), what
                assert np.array_equal(I, Io), what
            if nprobe == 1:                                           # lists of 0 and 1 rows: padding
                assert (Ifull[0] == -1).all() and (Dfull[0] == h16.NEG).all()
                if nq == 3:
                    assert (Ifull[1, 1:] == -1).all() and Ifull[1, 0] >= 0 and (Ifull[2, :50] >= 0).all()
            if nprobe == case.nlist and nq == 3:
                # every candidate: the equal rows tie and come out in list order, within a list and across two; then padding
                pos_of = {int(i): p for p, i in enumerate(case.ids)}
                Dall, Iall = h16.scan(case.halves, case.list_off, case.ids, Q, probes, bias, case.N)
                same = np.flatnonzero(bits(Dall[0, 1:]) == bits(Dall[0, :-1]))
                assert len(same) >= 43 and all(pos_of[int(Iall[0, s])] < pos_of[int(Iall[0, s + 1])] for s in same)
                D, I = case.scan(Q_d, dev(probes), bias_d, 2048)
                assert np.array_equal(bits(D[:, :case.N]), bits(Dall)) and np.array_equal(I[:, :case.N], Iall)
                assert (I[:, case.N:] == -1).all() and (D[:, case.N:] == h16.NEG).all()
                # the rows of subnormal halves and of -0 are among them with the restatement's scores
                lo = int(case.list_off[4])
                for p in (lo + 3, lo + 8, lo + 9):
                    assert case.ids[p] in Iall[0]


def test_selector_scan():
    d = 48
    case = scan_case(d)
    Q = unit_rows(3, d, 77)
    Q_d = dev(Q)
    probes = probe_sets(case.nlist, 3)[case.nlist + 4]
    bias_d, probes_d = gpu_bias(Q, case.c, probes), dev(probes)
    bias = bias_d.cpu().numpy()
    rng = np.random.default_rng(1)
    N, off = case.N, case.list_off
    for name, keep in (("empty", np.zeros(N, bool)), ("random", rng.random(N) < 0.5), ("sparse", rng.random(N) < 0.02), ("all", np.ones(N, bool))):
        keep_d = dev(keep_words(keep))
        for k in (1, 10, 100):
            Do, Io = h16.scan(case.halves, off, case.ids, Q, probes, bias, k, keep=keep)
            D, I = case.scan(Q_d, probes_d, bias_d, k, keep_d)
            assert np.array_equal(bits(D), bits(Do)) and np.array_equal(I, Io), (name, k)
        if name == "empty":
            assert (I == -1).all() and (D == h16.NEG).all()
        if name == "all":
            Dp, Ip = case.scan(Q_d, probes_d, bias_d, 100)
            assert np.array_equal(bits(D), bits(Dp)) and np.array_equal(I, Ip)


def test_bad_arguments_are_refused_without_a_launch():
    d = 48
    case = scan_case(d)
    Q_d = dev(unit_rows(2, d, 5))
    probes = probe_sets(case.nlist, 2)[3]
    bias_d, probes_d = gpu_bias(Q_d.cpu().numpy(), case.c, probes), dev(probes)
    lib = _lib.lib()
    keep_d = dev(keep_words(np.ones(case.N, bool)))
    need = lib.wise_ivfsq_scan_workspace_bytes(2, 3, 10)
    for kd in (None, keep_d):
        for kw, what in ((dict(d=24), b"d=24"), (dict(k=2049), b"k=2049"), (dict(ws_bytes=need - 1), b"workspace"), (dict(null="h"), b"null pointer"),
                         (dict(null="Q"), b"null pointer"), (dict(null="probes"), b"null pointer"), (dict(null="bias"), b"null pointer"),
                         (dict(null="D"), b"null pointer")):
            rc, D, I = case.raw_scan(Q_d, probes_d, bias_d, kw.pop("k", 10), kd, **kw)
            assert rc == WISE_E_INVALID and what in lib.wise_last_error(), (what, lib.wise_last_error())
            torch.cuda.synchronize()
            assert (D.cpu().numpy() == 7.0).all() and (I.cpu().numpy() == 7).all()      # nothing ran: the outputs are untouched
    st = _lib.stream_ptr()
    rc = lib.wise_ivfsq16_scan_sel(case.h_d.data_ptr(), case.N, d, case.off_d.data_ptr(), case.nlist, 0, Q_d.data_ptr(), 2, probes_d.data_ptr(),
                                   bias_d.data_ptr(), 3, 10, 0, Q_d.data_ptr(), Q_d.data_ptr(), Q_d.data_ptr(), need, st)
    assert rc == WISE_E_INVALID and b"null bitmap" in lib.wise_last_error()
    r = torch.zeros(8, 24, device="cuda")
    h = torch.zeros(8, 24, dtype=torch.float16, device="cuda")
    assert lib.wise_sq16_encode(r.data_ptr(), 8, 24, h.data_ptr(), st) == WISE_E_INVALID
    assert lib.wise_sq16_encode(0, 8, 16, h.data_ptr(), st) == WISE_E_INVALID
    p = torch.zeros(8, dtype=torch.int64, device="cuda")
    assert lib.wise_sq16_decode(h.data_ptr(), 8, p.data_ptr(), 8, p.data_ptr(), 1, r.data_ptr(), 24, r.data_ptr(), st) == WISE_E_INVALID
    assert lib.wise_sq16_decode(h.data_ptr(), 8, p.data_ptr(), 8, 0, 1, r.data_ptr(), 16, r.data_ptr(), st) == WISE_E_INVALID
    for fn, args in ((lib.wise_ivfsq16_range_count, (0.5, 0, 0)), (lib.wise_ivfsq16_range_fill, (0.5, 0, 0, 0))):
        head = (case.h_d.data_ptr(), case.N, 24, case.off_d.data_ptr(), case.nlist) + ((0,) if fn is lib.wise_ivfsq16_range_fill else ())
        assert fn(*head, Q_d.data_ptr(), 2, probes_d.data_ptr(), bias_d.data_ptr(), 3, *args, Q_d.data_ptr(), 1 << 20, st) == WISE_E_INVALID
        assert b"d=24" in lib.wise_last_error()


# ------------------------------------------------------------------------------------------------------------------ range_search
def test_range_count_fill_equal_the_prefix_of_the_scan():
    """Thresholds from the restatement's sorted scores: every query but the last has between 1 and 2047 hits, the last none (its
    bias is far below); the first threshold IS the score of a row, which is then no hit (strictly greater)."""
    lib = _lib.lib()
    d, nq = 48, 4
    case = scan_case(d)
    rng = np.random.default_rng(6)
    Q = unit_rows(nq, d, 31)
    probes = probe_sets(case.nlist, nq)[case.nlist + 4]
    nprobe = probes.shape[1]
    bias = rng.standard_normal((nq, nprobe)).astype(np.float32) * np.float32(0.1)
    bias[nq - 1] -= np.float32(100.0)
    bias[:, 11] = bias[:, 2]                                      # the list named twice has ONE bias, as q . c_l is
    per_q = h16.scores(case.halves, case.list_off, Q, probes, bias)
    srt = [np.sort(s)[::-1] for _, s in per_q]
    t_few = float(min(s[3] for s in srt[:-1]))                    # a row's score exactly
    t_many = float(max(s[min(1500, len(s) - 1)] for s in srt[:-1]))
    for t in (t_few, t_many):                                     # the restatement alone satisfies the test's premise
        n = [int((s > np.float32(t)).sum()) for s in srt]
        assert all(1 <= c <= 2047 for c in n[:-1]) and n[-1] == 0, (t, n)
    assert any((s == np.float32(t_few)).any() for s in srt)
    Q_d, probes_d, bias_d = dev(Q), dev(probes), dev(bias)
    Dk, Ik = case.scan(Q_d, probes_d, bias_d, K)                  # the scan's top-2048 answer ...
    Dr, Ir = h16.scan(case.halves, case.list_off, case.ids, Q, probes, bias, K)
    assert np.array_equal(bits(Dk), bits(Dr)) and np.array_equal(Ik, Ir)      # ... which is the restatement's
    need = lib.wise_ivfsq_range_workspace_bytes(case.N, case.nlist, nq, nprobe)
    assert need > 0
    st = _lib.stream_ptr()
    head = (case.h_d.data_ptr(), case.N, d, case.off_d.data_ptr(), case.nlist)
    mid = (Q_d.data_ptr(), nq, probes_d.data_ptr(), bias_d.data_ptr(), nprobe)
    for t in (t_few, t_many):
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        counts = torch.full((nq,), -7, dtype=torch.int64, device="cuda")
        _lib.check(lib.wise_ivfsq16_range_count(*head, *mid, t, 0, counts.data_ptr(), ws.data_ptr(), need, st), "count")
        c = counts.cpu().numpy()
        lims = np.concatenate([[0], np.cumsum(c)]).astype(np.int64)
        total = int(lims[-1])
        lims_d = dev(lims)
        for with_ids in (True, False):
            D = torch.full((total + 1,), 7.5, dtype=torch.float32, device="cuda")
            I = torch.full((total + 1,), -99, dtype=torch.int64, device="cuda")
            _lib.check(lib.wise_ivfsq16_range_fill(*head, case.ids_d.data_ptr() if with_ids else 0, *mid, t, lims_d.data_ptr(), D.data_ptr(),
                                                   I.data_ptr(), ws.data_ptr(), need, st), "fill")
            D, I = D.cpu().numpy(), I.cpu().numpy()
            assert D[total] == 7.5 and I[total] == -99                # nothing written past lims[nq]
            for q in range(nq):
                wd, wi = rr.prefix(Dk[q], Ik[q], t)
                s, p = D[lims[q]:lims[q + 1]], I[lims[q]:lims[q + 1]]
                assert c[q] == len(wd), (t, q, c[q], len(wd))
                pos = p if not with_ids else np.array([np.flatnonzero(case.ids == i)[0] for i in p], dtype=np.int64)
                o = rr.order(s, pos)
                assert np.array_equal(bits(s[o]), bits(wd)) and np.array_equal(case.ids[pos[o]], wi), (t, q, with_ids)
        assert c[-1] == 0 and (c[:-1] >= 1).all()


# ------------------------------------------------------------------------------------------------------------------ the index
@pytest.fixture(scope="module")
def built():
    """4,096 x 64 clustered rows in 16 lists: (X, ids, index trained and filled in one add)"""
    import ivfpq_ref

    N, d, nlist = 4096, 64, 16
    X = ivfpq_ref.clustered_unit_rows(N, d, 16, 0.35, 21)
    ids = np.random.default_rng(2).permutation(N).astype(np.int64) * 2 + 5
    idx = IVFSQfp16IPIndex(d, nlist)
    assert not idx.is_trained
    idx.train(X)
    assert idx.is_trained and idx.trained is None
    idx.add_with_ids(X, ids)
    return X, ids, idx


def index_reference(idx, Q, k, nprobe, keep=None):
    """the restatement on the index's own centroids, lists and probes"""
    c, halves, ids_s, off = idx.lists_host()
    probes = idx.probes_device(dev(Q), nprobe).cpu().numpy()
    bias = gpu_bias(Q, c, probes).cpu().numpy()
    return h16.scan(halves, off, ids_s, Q, probes, bias, k, keep=keep)


def test_index_chunked_adds_state_and_bytes(built):
    X, ids, idx = built
    N, d, nlist = len(X), idx.d, idx.nlist
    c, halves, ids_s, off = idx.lists_host()
    assert halves.dtype == np.float16 and halves.shape == (N, d)
    pos_of = {int(i): p for p, i in enumerate(ids)}
    rows = np.array([pos_of[int(i)] for i in ids_s])
    assert off[0] == 0 and off[-1] == N and (np.diff(off) > 0).all()
    for l in range(nlist):
        seg = rows[off[l]:off[l + 1]]
        assert (np.diff(seg) > 0).all() and ((X[seg] @ c.T).max(axis=1) - X[seg] @ c[l] < 1e-5).all()
    assert np.array_equal(hbits(halves), hbits(h16.encode(X[rows] - c[h16.list_of_rows(off)])))
    assert idx.ntotal == N and idx.hbm_bytes() == N * (2 * d + 8) + 8 * (nlist + 1) + 4 * nlist * d
    st = idx.state_host()
    assert set(st) == {"centroids", "halves", "ids", "list_off", "nprobe"}
    idx2 = IVFSQfp16IPIndex(d, nlist)
    idx2.set_centroids(c)
    assert idx2.is_trained
    for s, e in ((0, 1000), (1000, N)):                              # two chunks give the same lists as one add
        idx2.add_with_ids(X[s:e], ids[s:e])
    for u, v in zip(idx.lists_host(), idx2.lists_host()):
        assert u.tobytes() == v.tobytes()
    a, enc = idx.encode_rows(X[:500])
    at = np.array([{int(i): p for p, i in enumerate(ids_s)}[int(i)] for i in ids[:500]])
    assert enc.dtype == np.float16 and np.array_equal(hbits(enc), hbits(halves[at])) and np.array_equal(a, h16.list_of_rows(off)[at])
    with pytest.raises(ValueError):
        IVFSQfp16IPIndex(40, 4)
    with pytest.raises(RuntimeError):
        IVFSQfp16IPIndex(64, 4).add_with_ids(X[:4], ids[:4])


def test_index_search_reconstruct_and_selectors(built):
    X, ids, idx = built
    N, d = len(X), idx.d
    Q = X[:9] + np.float32(0.05) * unit_rows(9, d, 4)
    c, halves, ids_s, off = idx.lists_host()
    for nprobe, k in ((1, 10), (4, 100), (16, 10)):
        idx.nprobe = nprobe
        D, I = idx.search(Q, k)
        Do, Io = index_reference(idx, Q, k, nprobe)
        assert np.array_equal(bits(D), bits(Do)) and np.array_equal(I, Io), (nprobe, k)
    assert (I[:, 0] == ids[:9]).all()                                # every list probed: a row finds itself
    idx.make_direct_map(True)
    rec = idx.reconstruct_batch([int(ids_s[0]), int(ids_s[N - 1]), 4, int(ids_s[777])])
    want = h16.decode_rows(halves, off, c)
    assert np.array_equal(bits(rec[[0, 1, 3]]), bits(want[[0, N - 1, 777]])) and np.isnan(rec[2]).all()
    pos_of = {int(i): p for p, i in enumerate(ids)}
    assert np.abs(rec[0] - X[pos_of[int(ids_s[0])]]).max() <= 2.0 ** -11      # half a unit in the last place of a half below 1
    some = np.sort(ids[np.random.default_rng(3).permutation(N)[:300]])
    for sel, kept in ((IDSelectorBatch(some), np.isin(ids_s, some)),
                      (IDSelectorRange(1000, 3000), (ids_s >= 1000) & (ids_s < 3000)),
                      (IDSelectorNot(IDSelectorBatch(some)), ~np.isin(ids_s, some))):
        D, I = idx.search(Q, 10, params=SearchParametersIVF(sel=sel, nprobe=5))
        Do, Io = index_reference(idx, Q, 10, 5, keep=kept)
        assert np.array_equal(bits(D), bits(Do)) and np.array_equal(I, Io)
        assert np.isin(I[I >= 0], ids_s[kept]).all()
    assert idx.nprobe == 16                                          # the parameter's nprobe held for that call only


def test_index_range_search(built):
    X, ids, idx = built
    Q = X[[3, 500, 999, 1500, 2100, 2800, 3999]] + np.float32(0.01)
    idx.nprobe = 6
    Dk, Ik = idx.search(Q, K)
    t = float(max(Dk[q, 300] for q in range(len(Q))))
    lims, D, I = idx.range_search(Q, t)
    assert lims.dtype == np.int64 and lims.shape == (len(Q) + 1,) and lims[0] == 0 and lims[-1] == len(D) == len(I)
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.ndim == I.ndim == 1
    assert lims[-1] > 0 and (np.diff(lims) >= 0).all() and np.diff(lims).max() == 300
    for q in range(len(Q)):
        wd, wi = rr.prefix(Dk[q], Ik[q], t)
        assert np.array_equal(bits(D[lims[q]:lims[q + 1]]), bits(wd)) and np.array_equal(I[lims[q]:lims[q + 1]], wi)
    qd = dev(Q)
    whole = idx.range_search_device(qd, t)
    cut = idx.range_search_device(qd, t, chunk=2)
    assert whole[0].is_cuda and torch.equal(whole[0], cut[0]) and torch.equal(whole[1].view(torch.int32), cut[1].view(torch.int32))
    assert torch.equal(whole[2], cut[2]) and np.array_equal(whole[2].cpu().numpy(), I)
    some = np.sort(ids[np.random.default_rng(3).permutation(len(ids))[:len(ids) // 3]])
    ls, Ds, Is = idx.range_search(Q, t, params=SearchParametersIVF(sel=IDSelectorBatch(some)))
    for q in range(len(Q)):
        m = np.isin(I[lims[q]:lims[q + 1]], some)
        assert np.array_equal(Is[ls[q]:ls[q + 1]], I[lims[q]:lims[q + 1]][m]) and np.array_equal(bits(Ds[ls[q]:ls[q + 1]]), bits(D[lims[q]:lims[q + 1]][m]))
    l0, D0, I0 = idx.range_search(Q, float(Dk.max()))
    assert l0.tolist() == [0] * (len(Q) + 1) and D0.shape == (0,) and I0.shape == (0,)
    l1, D1, I1 = idx.range_search(Q, t, params=SearchParametersIVF(nprobe=16))
    assert idx.nprobe == 6 and (np.diff(l1) >= np.diff(lims)).all()
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            idx.range_search(Q, bad)
    idx.nprobe = 16


def test_remove_ids_leaves_the_index_of_the_kept_rows(built):
    X, ids, idx0 = built
    N, d, nlist = len(X), idx0.d, idx0.nlist
    c = idx0.lists_host()[0]
    gone = np.random.default_rng(8).random(N) < 0.3
    a, b = IVFSQfp16IPIndex(d, nlist), IVFSQfp16IPIndex(d, nlist)
    for i in (a, b):
        i.set_centroids(c)
    a.add_with_ids(X, ids)
    assert a.remove_ids(ids[gone], scratch_bytes=100 * 1024) == int(gone.sum())
    b.add_with_ids(X[~gone], ids[~gone])
    for u, v in zip(a.lists_host(), b.lists_host()):
        assert u.shape == v.shape and u.tobytes() == v.tobytes()
    assert a.ntotal == int((~gone).sum()) and a.hbm_bytes() == b.hbm_bytes()
    a.nprobe = b.nprobe = 5
    Q = X[:4]
    Da, Ia = a.search(Q, 10)
    Db, Ib = b.search(Q, 10)
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
    import ivfpq_ref
    from wise_amd.index.search_index_factory import SearchIndexFactory

    fdir, idir = tmp_path / "features", tmp_path / "index"
    fdir.mkdir()
    N, d, n_new = 3072, 64, 512
    ITYPE = "IndexIVFSQfp16"
    X = ivfpq_ref.clustered_unit_rows(N + n_new, d, 16, 0.35, 21)
    ids = np.arange(1, N + n_new + 1, dtype=np.int64)
    write_shard(fdir, 0, ids[:N], X[:N])
    si = SearchIndexFactory("video", "mlfoundations/open_clip/ViT-B-32/seeded-0", {"features_dir": fdir, "index_dir": idir})
    si.create_index(ITYPE)
    fn = si.get_index_filename(ITYPE)
    assert fn.name == "video-IndexIVFSQfp16.faiss" and faiss_io.index_fourcc(fn) == "IwSq"
    nlist = reference_nlist(N)
    assert struct.unpack_from("<i", fn.read_bytes(), 4 + 33 + 16 + 4 + 33 + 8 + 4 * nlist * d + 9)[0] == 4          # the file's qtype
    assert N * (2 * d + 8) < fn.stat().st_size < N * (2 * d + 8) + 4 * nlist * d + 8 * nlist + 512
    # the same build by hand: the file holds its lists, and the loaded index gives its answers
    mine = IVFSQfp16IPIndex(d, nlist)
    mine.train(X[:N][np.sort(np.random.default_rng(1234).permutation(N)[:min(N, 100 * nlist)])])
    mine.add_with_ids(X[:N], ids[:N])
    want_fn = tmp_path / "want.faiss"
    si._write_index_file(mine, want_fn)
    assert fn.read_bytes() == want_fn.read_bytes()
    assert si.load_index(ITYPE) is True and type(si.index) is IVFSQfp16IPIndex
    index = si.index
    assert index.nlist == nlist and index.ntotal == N and index.nprobe == 1
    index.nprobe = mine.nprobe = 8
    Q = X[:6]
    D, I = index.search(Q, 10)
    Dm, Im = mine.search(Q, 10)
    assert np.array_equal(bits(D), bits(Dm)) and np.array_equal(I, Im) and (I[:, 0] == np.arange(1, 7)).all()
    index.nprobe = nlist

    class Words:                                                     # the text tower gives 512 dimensions; this store has 64
        def extract_text_features(self, texts):
            return np.stack([X[len(t)] + np.float32(0.01) for t in texts])

    si.feature_extractor = Words()
    within = np.arange(100, 130, dtype=np.int64)
    dist, got = si.search("video", "dog", topk=5, within=within)
    assert dist.shape == (5,) and np.isin(got, within).all() and len(set(got.tolist())) == 5 and np.all(np.diff(dist) <= 0)
    both = si.search_batch("video", ["dog", "a cat"], topk=50, within=within)
    for _, i in both:
        assert set(i[:30].tolist()) == set(within.tolist()) and (i[30:] == -1).all()
    top_d, top_i = si.search("video", "dog", topk=200)
    t = float(top_d[40])
    rd, ri = si.search_range("video", "dog", t)
    wd, wi = rr.prefix(top_d, top_i, t)
    assert 1 <= len(rd) <= 40 and np.array_equal(bits(rd), bits(wd)) and np.array_equal(ri, wi)
    wide = np.arange(100, 900, dtype=np.int64)
    dw, iw = si.search_range("video", "dog", t, within=wide)
    m = np.isin(ri, wide)
    assert np.array_equal(iw, ri[m]) and np.array_equal(bits(dw), bits(rd[m]))
    del si.index, si.feature_extractor
    # update_index: the store loses its middle shard and gains a fourth
    write_shard(fdir, 3, ids[N:], X[N:])
    os.remove(fdir / "video-000001.tar")
    kept = np.concatenate([np.arange(0, 1024), np.arange(2048, N)])
    f = faiss_io.read_index(fn)
    want = IVFSQfp16IPIndex(d, nlist)
    want.set_centroids(f["centroids"])
    want.nprobe = f["nprobe"]
    want.add_with_ids(X[kept], ids[kept])
    want.add_with_ids(X[N:], ids[N:])
    si._write_index_file(want, want_fn)
    assert si.update_index(ITYPE) == (512, 1024)
    assert fn.read_bytes() == want_fn.read_bytes()
    assert si.update_index(ITYPE) == (0, 0)
    assert si.load_index(ITYPE) is True and si.index.ntotal == 2048 + 512
    si.index.nprobe = want.nprobe = 8
    Q = np.ascontiguousarray(X[[5, 2100, 3100, 1500]], dtype=np.float32)
    Da, Ia = si.index.search(Q, 10)
    Db, Ib = want.search(Q, 10)
    assert np.array_equal(bits(Da), bits(Db)) and np.array_equal(Ia, Ib)
    assert Ia[0, 0] == 6 and Ia[1, 0] == 2101 and Ia[2, 0] == 3101 and not np.isin(Ia, ids[1024:2048]).any()

"""-m gpu: IndexIVFSQ8 — wise_sq_* and wise_ivfsq_scan(_sel) through the C ABI against the numpy restatement (tests/ivfsq_ref.py),
bit for bit, then the index, its selectors and the SearchIndexFactory path on top of them."""
import numpy as np
import pytest
import torch

import ivfsq_ref as sq
from wise_amd import _lib
from wise_amd.index import faiss_io
from wise_amd.index.ivf_flat import reference_nlist
from wise_amd.index.ivf_sq import IVFSQIPIndex
from wise_amd.index.selector import IDSelectorBatch, IDSelectorNot, IDSelectorRange, SearchParametersIVF

pytestmark = pytest.mark.gpu

WISE_E_INVALID = -1


def unit_rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def gpu_train(resid):
    n, d = resid.shape
    r_d, out = dev(resid), torch.empty(2 * d, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().wise_sq_train(r_d.data_ptr(), n, d, out.data_ptr(), _lib.stream_ptr()), "wise_sq_train")
    t = out.cpu().numpy()
    return t[:d], t[d:]


def gpu_encode(resid, vmin, vdiff):
    n, d = resid.shape
    r_d, t_d = dev(resid), dev(np.concatenate([vmin, vdiff]))
    codes = torch.empty(n, d, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().wise_sq_encode(r_d.data_ptr(), t_d.data_ptr(), n, d, codes.data_ptr(), _lib.stream_ptr()), "wise_sq_encode")
    return codes.cpu().numpy()


def gpu_decode(codes, pos, list_off, c, vmin, vdiff):
    N, d = codes.shape
    a = [dev(x) for x in (codes, pos, list_off, c, np.concatenate([vmin, vdiff]))]
    out = torch.empty(len(pos), d, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().wise_sq_decode(a[0].data_ptr(), N, a[1].data_ptr(), len(pos), a[2].data_ptr(), len(c), a[3].data_ptr(),
                                         a[4].data_ptr(), d, out.data_ptr(), _lib.stream_ptr()), "wise_sq_decode")
    return out.cpu().numpy()


def gpu_query(Q, vmin, vdiff):
    nq, d = Q.shape
    Q_d, t_d = dev(Q), dev(np.concatenate([vmin, vdiff]))
    W = torch.empty(nq, d, dtype=torch.float32, device="cuda")
    q0 = torch.empty(nq, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().wise_sq_query(Q_d.data_ptr(), t_d.data_ptr(), nq, d, W.data_ptr(), q0.data_ptr(), _lib.stream_ptr()), "wise_sq_query")
    return W, q0


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
    """An index on the device: codes, list offsets, ids, and what a query needs."""

    def __init__(self, codes, list_off, ids, c, vmin, vdiff):
        self.codes, self.list_off, self.ids, self.c, self.vmin, self.vdiff = codes, list_off, ids, c, vmin, vdiff
        self.N, self.d = codes.shape
        self.nlist = len(list_off) - 1
        self.codes_d, self.off_d, self.ids_d = dev(codes), dev(list_off), dev(ids)

    def raw_scan(self, W_d, q0_d, probes_d, bias_d, k, keep_d=None, ws_bytes=None, codes_ptr=None, d=None):
        lib = _lib.lib()
        nq, nprobe = probes_d.shape
        need = lib.wise_ivfsq_scan_workspace_bytes(nq, nprobe, k)
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
        D = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
        I = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
        head = (self.codes_d.data_ptr() if codes_ptr is None else codes_ptr, self.N, self.d if d is None else d, self.off_d.data_ptr(),
                self.nlist, self.ids_d.data_ptr(), W_d.data_ptr(), q0_d.data_ptr(), nq, probes_d.data_ptr(), bias_d.data_ptr(), nprobe, k)
        tail = (D.data_ptr(), I.data_ptr(), ws.data_ptr(), need if ws_bytes is None else ws_bytes, _lib.stream_ptr())
        rc = lib.wise_ivfsq_scan(*head, *tail) if keep_d is None else lib.wise_ivfsq_scan_sel(*head, keep_d.data_ptr(), *tail)
        return rc, D, I

    def scan(self, W_d, q0_d, probes_d, bias_d, k, keep_d=None):
        rc, D, I = self.raw_scan(W_d, q0_d, probes_d, bias_d, k, keep_d)
        _lib.check(rc, "wise_ivfsq_scan")
        return D.cpu().numpy(), I.cpu().numpy()


LENGTHS = (0, 1, 2, 63, 64, 65, 257, 1500)


def scan_case(d, fill=None):
    """lists of LENGTHS rows of random codes (fill: every code that value); duplicated rows in the longest list; one dimension
    whose range is zero; ids a permutation"""
    rng = np.random.default_rng(100 + d)
    list_off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    N = int(list_off[-1])
    codes = rng.integers(0, 256, (N, d), dtype=np.uint8) if fill is None else np.full((N, d), fill, dtype=np.uint8)
    lo = int(list_off[-2])
    codes[lo + 700:lo + 760] = codes[lo + 10:lo + 70]            # equal rows: the first in list order wins
    c = unit_rows(len(LENGTHS), d, d + 1)
    vmin = (-rng.uniform(0.05, 0.4, d)).astype(np.float32)
    vdiff = rng.uniform(0.1, 0.8, d).astype(np.float32)
    vdiff[5] = 0
    codes[:, 5] = 0 if fill is None else fill
    ids = rng.permutation(N).astype(np.int64) * 7 + 1
    return Case(codes, list_off, ids, c, vmin, vdiff)


def probe_sets(nlist, nq):
    """nprobe -> [nq, nprobe]: 1 probe = the lists of 0 / 1 / 2 rows (padding), more = a rotation of the lists, nlist + 3 with -1s"""
    out = {1: np.array([[0], [1], [2]], dtype=np.int64)[:nq]}
    rot = np.stack([np.roll(np.arange(nlist, dtype=np.int64)[::-1], q) for q in range(nq)])
    out[5] = rot[:, :5].copy()
    out[nlist] = rot.copy()
    wide = np.full((nq, nlist + 3), -1, dtype=np.int64)
    wide[:, [0, 2, 3, 5, 6, 7, 9, 10]] = rot
    out[nlist + 3] = wide
    return out


def prefix(Dfull, Ifull, k):
    nq, kf = Dfull.shape
    D = np.full((nq, k), sq.NEG, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    D[:, :min(k, kf)], I[:, :min(k, kf)] = Dfull[:, :k], Ifull[:, :k]
    return D, I


@pytest.mark.parametrize("d", [16, 48])
def test_train_encode_and_decode_give_the_restatements_bits(d):
    for n in (1, 63, 64, 65, 1000):
        rng = np.random.default_rng(n + d)
        resid = (rng.standard_normal((n, d)) * rng.uniform(0.01, 2.0, d)).astype(np.float32)
        if n > 1:
            resid[:, 3] = np.float32(-0.125)                      # a dimension that never varies
        vmin, vdiff = sq.train(resid)
        gmin, gdiff = gpu_train(resid)
        assert np.array_equal(bits(gmin), bits(vmin)) and np.array_equal(bits(gdiff), bits(vdiff)), (d, n)
        # rows beyond the trained range too: they clamp
        wide = np.concatenate([resid, resid * np.float32(1.5), vmin[None, :] - np.float32(1.0), (vmin + vdiff)[None, :] + np.float32(1.0)])
        codes = sq.encode(wide, vmin, vdiff)
        assert np.array_equal(gpu_encode(wide, vmin, vdiff), codes), (d, n)
        assert (codes[-2] == 0).all() and (codes[-1][vdiff > 0] == 255).all() and (codes[:, vdiff == 0] == 0).all()
        N = len(codes)
        list_off = np.array([0, N // 3, N // 3, N], dtype=np.int64)   # three lists, the middle one empty
        c = unit_rows(3, d, n)
        pos = np.concatenate([np.arange(N), [-1, N, N + 5]]).astype(np.int64)
        got = gpu_decode(codes, pos, list_off, c, vmin, vdiff)
        assert np.array_equal(bits(got[:N]), bits(sq.decode_rows(codes, list_off, c, vmin, vdiff))), (d, n)
        assert np.isnan(got[N:]).all()


@pytest.mark.parametrize("d", [16, 48, 512, 1024])
def test_scan_is_bit_equal_to_the_restatement(d):
    case = scan_case(d)
    Q3 = unit_rows(3, d, d + 9) * np.float32(1.3)
    for nq in (1, 3):
        Q = Q3[:nq]
        W_d, q0_d = gpu_query(Q, case.vmin, case.vdiff)
        W, q0 = sq.query(Q, case.vmin, case.vdiff)
        assert np.array_equal(bits(W_d.cpu().numpy()), bits(W)) and np.array_equal(bits(q0_d.cpu().numpy()), bits(q0)), (d, nq)
        for nprobe, probes in probe_sets(case.nlist, nq).items():
            bias_d = gpu_bias(Q, case.c, probes)
            bias = bias_d.cpu().numpy()
            Dfull, Ifull = sq.scan(case.codes, case.list_off, case.ids, W, q0, probes, bias, 100)
            for k in (1, 10, 100):
                D, I = case.scan(W_d, q0_d, dev(probes), bias_d, k)
                Do, Io = prefix(Dfull, Ifull, k)
                what = f"d={d} nq={nq} nprobe={nprobe} k={k}"
                assert np.array_equal(bits(D), bits(Do)), what
                assert np.array_equal(I, Io), what
            if nprobe == 1:                                           # lists of 0, 1 and 2 rows: padding from the first slot on
                assert (Ifull[0] == -1).all() and (Dfull[0] == sq.NEG).all()
                if nq == 3:
                    assert (Ifull[1, 1:] == -1).all() and (Ifull[2, 2:] == -1).all() and (Ifull[2, :2] >= 0).all()
            if nprobe == case.nlist and nq == 3:
                # the equal rows tie and come out in list order
                pos_of = {int(i): p for p, i in enumerate(case.ids)}
                Dall, Iall = sq.scan(case.codes, case.list_off, case.ids, W, q0, probes, bias, case.N)
                same = np.flatnonzero(bits(Dall[0, 1:]) == bits(Dall[0, :-1]))
                assert len(same) >= 60 and all(pos_of[int(Iall[0, s])] < pos_of[int(Iall[0, s + 1])] for s in same)
                D, I = case.scan(W_d, q0_d, dev(probes), bias_d, 2048)
                assert np.array_equal(bits(D[:, :case.N]), bits(Dall)) and np.array_equal(I[:, :case.N], Iall)
                assert (I[:, case.N:] == -1).all() and (D[:, case.N:] == sq.NEG).all()


@pytest.mark.parametrize("fill", [0, 255])
@pytest.mark.parametrize("d", [16, 512])
def test_scan_of_constant_codes(d, fill):
    """every code 0 / every code 255: a sign or widening mistake shows; within a list every score is equal and list order decides"""
    case = scan_case(d, fill=fill)
    Q = unit_rows(3, d, d + fill)
    W_d, q0_d = gpu_query(Q, case.vmin, case.vdiff)
    W, q0 = sq.query(Q, case.vmin, case.vdiff)
    probes = probe_sets(case.nlist, 3)[case.nlist + 3]
    bias_d = gpu_bias(Q, case.c, probes)
    Do, Io = sq.scan(case.codes, case.list_off, case.ids, W, q0, probes, bias_d.cpu().numpy(), 100)
    D, I = case.scan(W_d, q0_d, dev(probes), bias_d, 100)
    assert np.array_equal(bits(D), bits(Do)) and np.array_equal(I, Io)
    x = sq.decode_rows(case.codes, case.list_off, case.c, case.vmin, case.vdiff, np.float64) @ Q[0].astype(np.float64)
    pos_of = {int(i): p for p, i in enumerate(case.ids)}
    assert abs(float(D[0, 0]) - x[pos_of[int(I[0, 0])]]) < 1e-4       # and it is the decoded row's inner product


def test_selector_scan():
    d = 48
    case = scan_case(d)
    Q = unit_rows(3, d, 77)
    W_d, q0_d = gpu_query(Q, case.vmin, case.vdiff)
    W, q0 = sq.query(Q, case.vmin, case.vdiff)
    probes = probe_sets(case.nlist, 3)[case.nlist + 3]
    bias_d, probes_d = gpu_bias(Q, case.c, probes), dev(probes)
    bias = bias_d.cpu().numpy()
    rng = np.random.default_rng(1)
    N, off = case.N, case.list_off
    one = np.zeros(N, bool)
    one[int(off[-2]) + 1234] = True
    cleared = np.ones(N, bool)
    cleared[off[-2]:off[-1]] = False                             # the list of 1500 rows
    sparse = rng.random(N) < 0.02                                # most wave-loads hold no selected row
    for name, keep in (("empty", np.zeros(N, bool)), ("one", one), ("cleared", cleared), ("sparse", sparse), ("all", np.ones(N, bool))):
        keep_d = dev(keep_words(keep))
        for k in (1, 10, 100):
            Do, Io = sq.scan(case.codes, off, case.ids, W, q0, probes, bias, k, keep=keep)
            D, I = case.scan(W_d, q0_d, probes_d, bias_d, k, keep_d)
            assert np.array_equal(bits(D), bits(Do)) and np.array_equal(I, Io), (name, k)
        if name == "empty":
            assert (I == -1).all() and (D == sq.NEG).all()
        if name == "one":
            assert (I[:, 0] == case.ids[int(off[-2]) + 1234]).all() and (I[:, 1:] == -1).all()
        if name == "all":
            Dp, Ip = case.scan(W_d, q0_d, probes_d, bias_d, 100)
            assert np.array_equal(bits(D), bits(Dp)) and np.array_equal(I, Ip)


def test_bad_arguments_are_refused_without_a_launch():
    d = 48
    case = scan_case(d)
    Q = unit_rows(2, d, 5)
    W_d, q0_d = gpu_query(Q, case.vmin, case.vdiff)
    probes = probe_sets(case.nlist, 2)[5]
    bias_d, probes_d = gpu_bias(Q, case.c, probes), dev(probes)
    lib = _lib.lib()
    keep_d = dev(keep_words(np.ones(case.N, bool)))
    for kd in (None, keep_d):
        rc, D, I = case.raw_scan(W_d, q0_d, probes_d, bias_d, 10, kd, d=20)
        assert rc == WISE_E_INVALID and b"d=20" in lib.wise_last_error()
        rc, D, I = case.raw_scan(W_d, q0_d, probes_d, bias_d, 10, kd, codes_ptr=case.codes_d.data_ptr() + 4)
        assert rc == WISE_E_INVALID and b"16-byte aligned" in lib.wise_last_error()
        need = lib.wise_ivfsq_scan_workspace_bytes(2, 5, 10)
        rc, D, I = case.raw_scan(W_d, q0_d, probes_d, bias_d, 10, kd, ws_bytes=need - 1)
        assert rc == WISE_E_INVALID and b"workspace" in lib.wise_last_error()
        rc, D, I = case.raw_scan(W_d, q0_d, probes_d, bias_d, 4096, kd)
        assert rc == WISE_E_INVALID and b"k=4096" in lib.wise_last_error()
        torch.cuda.synchronize()
        assert (D.cpu().numpy() == 7.0).all() and (I.cpu().numpy() == 7).all()      # nothing ran: the outputs are untouched
    assert lib.wise_ivfsq_scan_workspace_bytes(2, 5, 4096) == 0 and lib.wise_ivfsq_scan_workspace_bytes(2, 4096, 10) == 0
    r = torch.zeros(8, 20, device="cuda")
    t = torch.zeros(40, device="cuda")
    assert lib.wise_sq_train(r.data_ptr(), 8, 20, t.data_ptr(), _lib.stream_ptr()) == WISE_E_INVALID
    assert lib.wise_sq_query(r.data_ptr(), t.data_ptr(), 8, 20, r.data_ptr(), t.data_ptr(), _lib.stream_ptr()) == WISE_E_INVALID


# ------------------------------------------------------------------------------------------------------------------ the index
@pytest.fixture(scope="module")
def built():
    """4,096 x 64 clustered rows in 16 lists: (X, ids, index trained and filled in one add)"""
    import ivfpq_ref

    N, d, nlist = 4096, 64, 16
    X = ivfpq_ref.clustered_unit_rows(N, d, 16, 0.35, 21)
    ids = np.random.default_rng(2).permutation(N).astype(np.int64) * 2 + 5
    idx = IVFSQIPIndex(d, nlist)
    assert not idx.is_trained
    idx.train(X)
    assert idx.is_trained
    idx.add_with_ids(X, ids)
    return X, ids, idx


def index_reference(idx, Q, k, nprobe, keep=None):
    """the restatement on the index's own centroids, ranges, lists and probes"""
    c, trained, codes, ids_s, off = idx.lists_host()
    d = idx.d
    probes = idx.probes_device(dev(Q), nprobe).cpu().numpy()
    bias = gpu_bias(Q, c, probes).cpu().numpy()
    W, q0 = sq.query(Q, trained[:d], trained[d:])
    return sq.scan(codes, off, ids_s, W, q0, probes, bias, k, keep=keep)


def test_index_training_and_chunked_adds(built):
    X, ids, idx = built
    N, d, nlist = len(X), idx.d, idx.nlist
    c, trained, codes, ids_s, off = idx.lists_host()
    # the ranges are the exact min / range of the training residuals, the codes the restatement's
    pos_of = {int(i): p for p, i in enumerate(ids)}
    rows = np.array([pos_of[int(i)] for i in ids_s])
    assert off[0] == 0 and off[-1] == N and (np.diff(off) > 0).all()
    for l in range(nlist):                                           # every row sits in the list of its best centroid, in order of insertion
        seg = rows[off[l]:off[l + 1]]
        assert (np.diff(seg) > 0).all() and ((X[seg] @ c.T).max(axis=1) - X[seg] @ c[l] < 1e-5).all()
    resid = X[rows] - c[sq.list_of_rows(off)]
    vmin, vdiff = sq.train(resid)
    assert np.array_equal(bits(trained[:d]), bits(vmin)) and np.array_equal(bits(trained[d:]), bits(vdiff))
    assert np.array_equal(codes, sq.encode(resid, vmin, vdiff))
    assert idx.ntotal == N and idx.hbm_bytes() == N * (d + 8) + 8 * (nlist + 1) + 4 * nlist * d + 8 * d
    # three uneven chunks give the same lists as one add
    idx2 = IVFSQIPIndex(d, nlist)
    idx2.set_centroids(c)
    idx2.set_trained(trained[:d], trained[d:])
    for s, e in ((0, 1000), (1000, 1001), (1001, N)):
        idx2.add_with_ids(X[s:e], ids[s:e])
    for u, v in zip(idx.lists_host(), idx2.lists_host()):
        assert np.array_equal(u, v)
    with pytest.raises(ValueError):
        idx2.set_trained(trained[:d], trained[:d - 1])
    with pytest.raises(ValueError):
        IVFSQIPIndex(40, 4)
    with pytest.raises(RuntimeError):
        IVFSQIPIndex(64, 4).add_with_ids(X[:4], ids[:4])


def test_index_search_reconstruct_and_selectors(built):
    X, ids, idx = built
    N, d = len(X), idx.d
    Q = X[:9] + np.float32(0.05) * unit_rows(9, d, 4)
    c, trained, codes, ids_s, off = idx.lists_host()
    for nprobe, k in ((1, 10), (4, 100), (16, 10)):
        idx.nprobe = nprobe
        D, I = idx.search(Q, k)
        Do, Io = index_reference(idx, Q, k, nprobe)
        assert np.array_equal(bits(D), bits(Do)) and np.array_equal(I, Io), (nprobe, k)
    assert (I[:, 0] == ids[:9]).all()                                # every list probed: a row finds itself
    # reconstruct_batch: the decoded rows, NaN for an unknown id
    idx.make_direct_map(True)
    rec = idx.reconstruct_batch([int(ids_s[0]), int(ids_s[N - 1]), 4, int(ids_s[777])])
    want = sq.decode_rows(codes, off, c, trained[:d], trained[d:])
    assert np.array_equal(bits(rec[[0, 1, 3]]), bits(want[[0, N - 1, 777]])) and np.isnan(rec[2]).all()
    pos_of = {int(i): p for p, i in enumerate(ids)}
    assert np.abs(rec[0] - X[pos_of[int(ids_s[0])]]).max() <= trained[d:].max() / 510 * 1.001
    # selectors through search(params=): the restatement restricted to the kept rows
    some = np.sort(ids[np.random.default_rng(3).permutation(N)[:300]])
    for sel, kept in ((IDSelectorBatch(some), np.isin(ids_s, some)),
                      (IDSelectorRange(1000, 3000), (ids_s >= 1000) & (ids_s < 3000)),
                      (IDSelectorNot(IDSelectorBatch(some)), ~np.isin(ids_s, some))):
        D, I = idx.search(Q, 10, params=SearchParametersIVF(sel=sel, nprobe=5))
        Do, Io = index_reference(idx, Q, 10, 5, keep=kept)
        assert np.array_equal(bits(D), bits(Do)) and np.array_equal(I, Io)
        assert np.isin(I[I >= 0], ids_s[kept]).all()
    assert idx.nprobe == 16                                          # the parameter's nprobe held for that call only


def test_search_index_builds_loads_and_filters(tmp_path):
    import ivfpq_ref
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    from wise_amd.index.search_index_factory import SearchIndexFactory

    fdir, idir = tmp_path / "features", tmp_path / "index"
    fdir.mkdir()
    N, d = 4096, 64
    X = ivfpq_ref.clustered_unit_rows(N, d, 16, 0.35, 21)
    st = FeatureStoreFactory.create_store(FeatureStoreType.WEBDATASET, "video", str(fdir))
    st.enable_write(2048, 20 * 1024 * 1024)
    for i in range(N):
        st.add(i + 1, X[i:i + 1])
    st.close()
    si = SearchIndexFactory("video", "mlfoundations/open_clip/ViT-B-32/seeded-0", {"features_dir": fdir, "index_dir": idir})
    si.create_index("IndexIVFSQ8")
    fn = si.get_index_filename("IndexIVFSQ8")
    assert fn.name == "video-IndexIVFSQ8.faiss" and faiss_io.index_fourcc(fn) == "IwSq"
    assert fn.stat().st_size < N * d * 4 // 2                         # one byte per dimension, not four
    # the same build by hand: the file holds its lists, and the loaded index gives its answers
    nlist = reference_nlist(N)
    mine = IVFSQIPIndex(d, nlist)
    mine.train(X[np.sort(np.random.default_rng(1234).permutation(N)[:min(N, 100 * nlist)])])
    mine.add_with_ids(X, np.arange(1, N + 1, dtype=np.int64))
    f = faiss_io.read_ivf_sq_ip(fn)
    mc, mt, mcodes, mids, moff = mine.lists_host()
    assert np.array_equal(mc, f["centroids"]) and np.array_equal(bits(mt), bits(f["trained"])) and np.array_equal(moff, f["list_off"])
    assert np.array_equal(mcodes[np.argsort(mids)], f["codes"][np.argsort(f["ids"])])
    for l in range(nlist):
        assert np.array_equal(np.sort(mids[moff[l]:moff[l + 1]]), np.sort(f["ids"][moff[l]:moff[l + 1]]))
    assert si.load_index("IndexIVFSQ8") is True and isinstance(si.index, IVFSQIPIndex)
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
            return np.stack([unit_rows(1, d, len(t))[0] for t in texts])

    si.feature_extractor = Words()
    within = np.arange(100, 130, dtype=np.int64)
    dist, ids = si.search("video", "dog", topk=5, within=within)
    assert dist.shape == (5,) and np.isin(ids, within).all() and len(set(ids.tolist())) == 5 and np.all(np.diff(dist) <= 0)
    both = si.search_batch("video", ["dog", "a cat"], topk=50, within=within)
    assert len(both) == 2
    for _, i in both:
        assert set(i[:30].tolist()) == set(within.tolist()) and (i[30:] == -1).all()
    plain = si.search("video", "dog", topk=5)
    assert plain[1].shape == (5,) and (plain[1] >= 1).all()

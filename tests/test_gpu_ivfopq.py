"""-m gpu: IndexIVFOPQ — the wise_opq_* kernels through the C ABI against float64 (tests/ivfopq_ref.py), then the index classes
and the SearchIndexFactory path on top of them.  Every bound below is the standard one for the arithmetic the header states
(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: a sum of n products accumulated one term at a time in
precision u is off by at most gamma_n sum |x_i y_i|, gamma_n = n u / (1 - n u)); there is no fitted constant."""
import json

import numpy as np
import pytest
import torch

import ivfopq_ref
import ivfpq_ref
import ivfpq_refine_ref as rr
from oracle import ip_topk_ref
from wise_amd import _lib
from wise_amd.index.ivf_flat import reference_nlist
from wise_amd.index.ivf_pq import (DEFAULT_K_FACTOR, IVFOPQIPIndex, IVFOPQRefineIPIndex, IVFPQIPIndex, IVFPQRefineIPIndex)

pytestmark = pytest.mark.gpu

U32, U64 = 2.0 ** -24, 2.0 ** -53


def gamma(n, u):
    return n * u / (1.0 - n * u)


def unit_rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def orthonormal(d, seed):
    return ivfopq_ref.procrustes(np.random.default_rng(seed).standard_normal((d, d))).astype(np.float32)


def gpu_rotate(x_d, R_d):
    out = torch.full_like(x_d, float("nan"))
    _lib.check(_lib.lib().wise_opq_rotate(x_d.data_ptr(), R_d.data_ptr(), x_d.shape[0], x_d.shape[1], out.data_ptr(), _lib.stream_ptr()),
               "wise_opq_rotate")
    return out


# --------------------------------------------------------------------------------------------------------------------- rotate
@pytest.mark.parametrize("n", [1, 7, 100000])
@pytest.mark.parametrize("d", [64, 512, 768, 1024])
def test_rotate_within_the_chain_bound_and_deterministic(d, n):
    rng = np.random.default_rng(1000 * d + n)
    x = rng.standard_normal((n, d)).astype(np.float32)
    R = orthonormal(d, d)
    x_d, R_d = dev(x), dev(R)
    got_d = gpu_rotate(x_d, R_d)
    again = gpu_rotate(x_d, R_d)
    assert torch.equal(got_d.view(torch.int32), again.view(torch.int32))                  # the same bits, call after call
    got = got_d.cpu().numpy()
    assert np.isfinite(got).all()
    R64, worst = R.astype(np.float64), 0.0
    for s in range(0, n, 8192):                                                           # every row, 8192 at a time
        xs = x[s:s + 8192].astype(np.float64)
        err = np.abs(got[s:s + 8192].astype(np.float64) - xs @ R64.T)
        bound = gamma(d, U32) * (np.abs(xs) @ np.abs(R64).T)
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        assert (err <= bound).all()
    print(f"rotate d={d} n={n}: max err / bound {worst:.4f}")
    # a row's result depends on the row and on R alone: not on n, nor on where the row sits in its tile
    one = gpu_rotate(dev(x[n - 1:n]), R_d).cpu().numpy()
    assert np.array_equal(one.view(np.uint32), got[n - 1:n].view(np.uint32))
    # R = I returns x exactly
    eye = gpu_rotate(x_d, torch.eye(d, device="cuda")).cpu().numpy()
    assert np.array_equal(eye, x)


def test_rotate_refuses_what_it_does_not_serve():
    lib = _lib.lib()
    x = torch.zeros(4 * 1028, dtype=torch.float32, device="cuda")
    R = torch.zeros(1028 * 1028, dtype=torch.float32, device="cuda")
    out = torch.zeros_like(x)
    assert lib.wise_opq_rotate(x.data_ptr(), R.data_ptr(), 4, 1028, out.data_ptr(), 0) == -3           # d > 1024
    assert b"d <= 1024" in lib.wise_last_error()
    assert lib.wise_opq_rotate(x.data_ptr(), R.data_ptr(), 4, 1026, out.data_ptr(), 0) == -3           # d % 4
    assert lib.wise_opq_rotate(x.data_ptr(), R.data_ptr(), 4, 64, x.data_ptr(), 0) == -1               # out aliases x
    assert b"alias" in lib.wise_last_error()
    assert lib.wise_opq_rotate(x.data_ptr() + 4, R.data_ptr(), 4, 64, out.data_ptr(), 0) == -1         # alignment
    assert lib.wise_opq_rotate(0, R.data_ptr(), 0, 64, 0, 0) == 0                                      # no rows: nothing to do
    with pytest.raises(ValueError, match=r"\[4, 1024\]"):
        IVFOPQIPIndex(2048, 10, 64)
    with pytest.raises(ValueError):
        IVFOPQIPIndex(512, 10, 7)
    with pytest.raises(ValueError, match="stores are 8"):
        IVFOPQRefineIPIndex(512, 10, 64, 4)
    idx = IVFOPQIPIndex(64, 10, 8)
    with pytest.raises(ValueError, match=r"expected \[64,64\]"):
        idx.set_rotation(np.eye(32, dtype=np.float32))


# --------------------------------------------------------------------------------------------------------------------- corr
@pytest.mark.parametrize("n,d,m", [(10000, 64, 8), (5000, 512, 64), (4097, 24, 4), (300, 768, 8)])
def test_corr_within_the_summation_bound_and_deterministic(n, d, m):
    lib = _lib.lib()
    rng = np.random.default_rng(n + d)
    x = rng.standard_normal((n, d)).astype(np.float32)
    cb = rng.standard_normal((m, 256, d // m)).astype(np.float32)
    codes = rng.integers(0, 256, (n, m)).astype(np.uint8)
    x_d, cb_d, c_d = dev(x), dev(cb), dev(codes)
    need = lib.wise_opq_corr_workspace_bytes(n, d)
    assert need >= ((n + 4095) // 4096) * d * d * 8
    outs = []
    for fill in (0x00, 0xFF):                                                             # whatever the workspace held before
        ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
        M = torch.full((d, d), float("nan"), dtype=torch.float64, device="cuda")
        _lib.check(lib.wise_opq_corr(c_d.data_ptr(), cb_d.data_ptr(), x_d.data_ptr(), n, d, m, M.data_ptr(), ws.data_ptr(), ws.numel(),
                                     _lib.stream_ptr()), "wise_opq_corr")
        outs.append(M.cpu().numpy())
    assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64))               # the same bits
    cw = ivfopq_ref.codewords(codes, cb)
    want = ivfopq_ref.correlation(codes, cb, x)
    bound = gamma(n, U64) * (np.abs(cw).T @ np.abs(x.astype(np.float64)))                 # the products are exact in fp64
    err = np.abs(outs[0] - want)
    print(f"corr n={n} d={d} m={m}: max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.4f}")
    assert (err <= bound).all()
    assert lib.wise_opq_corr(c_d.data_ptr(), cb_d.data_ptr(), x_d.data_ptr(), n, d, m, M.data_ptr(), ws.data_ptr(), need - 1, 0) == -2
    assert b"workspace" in lib.wise_last_error()


# --------------------------------------------------------------------------------------------------------------------- index
def search_and_probes(idx, Q, k):
    """idx.search(Q, k) and the probes that very search took from its coarse stage (the index's own state: a second call of
    the coarse stage is not what the search scanned)."""
    seen, real = [], idx._coarse.probes_device
    idx._coarse.probes_device = lambda q, nprobe: seen.append(real(q, nprobe)) or seen[-1]
    try:
        D, I = idx.search(Q, k)
    finally:
        del idx._coarse.probes_device
    assert len(seen) == 1
    return D, I, seen[0].contiguous()


def gpu_tables(idx, Q_d, probes_d):
    """bias from the queries and the table from the index's ROTATED queries, as its search computes them"""
    lib, st = _lib.lib(), _lib.stream_ptr()
    nq, nprobe = probes_d.shape
    bias = torch.empty(nq, nprobe, dtype=torch.float32, device="cuda")
    _lib.check(lib.wise_pq_bias(Q_d.data_ptr(), idx.centroids.data_ptr(), probes_d.data_ptr(), nq, nprobe, idx.nlist, idx.d,
                                bias.data_ptr(), st), "wise_pq_bias")
    Qr = gpu_rotate(Q_d, idx.rotation)
    lut = torch.empty(nq, idx.m, 256, dtype=torch.float32, device="cuda")
    _lib.check(lib.wise_pq_lut(Qr.data_ptr(), idx.codebooks.data_ptr(), nq, idx.d, idx.m, lut.data_ptr(), st), "wise_pq_lut")
    return bias.cpu().numpy(), lut.cpu().numpy(), Qr.cpu().numpy()


def small_set():
    N, d = 20000, 64
    X = ivfopq_ref.decaying_spectrum_rows(N, d, 140, 0.5, seed=31)
    Q = unit_rows(16, d, 4) * 0.2 + X[100:116]
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    return X, Q, np.arange(N, dtype=np.int64) * 3 + 11


def test_index_search_equals_the_restatement_on_its_own_state():
    X, Q, ids = small_set()
    N, d, nlist, m, k = X.shape[0], X.shape[1], 100, 16, 10
    idx = IVFOPQIPIndex(d, nlist, m)
    assert isinstance(idx, IVFPQIPIndex) and (idx.opq_niter, idx.opq_niter_pq, idx.niter) == (50, 4, 10) and idx.rotation is None
    idx.opq_niter = 6
    with pytest.raises(RuntimeError):
        idx.add_with_ids(X, ids)
    idx._coarse.train(dev(X))
    idx.set_codebooks(np.zeros((m, 256, d // m), np.float32))
    assert not idx.is_trained                                              # centroids and codebooks but no rotation yet
    idx.train(X)
    assert idx.is_trained and idx.rotation.shape == (d, d) and idx.rotation.dtype == torch.float32 and idx.rotation.is_cuda
    for s in range(0, N, 7000):
        idx.add_with_ids(X[s:s + 7000], ids[s:s + 7000])
    assert idx.ntotal == N
    c, cb, codes, ids_s, off = idx.lists_host()
    R = idx.rotation.cpu().numpy()
    assert np.abs(R.astype(np.float64) @ R.astype(np.float64).T - np.eye(d)).max() <= 1e-5
    assert np.abs(R - np.eye(d)).max() > 1e-2                              # it did learn something
    assert idx.hbm_bytes() == N * (m + 8) + (nlist + 1) * 8 + nlist * d * 4 + m * 256 * (d // m) * 4 + d * d * 4
    # the codes are those of the rotated residuals: wise_pq_encode fed by wise_opq_rotate
    Xs = X[(ids_s - 11) // 3]
    resid_d = dev(Xs - c[ivfpq_ref.list_of_rows(off)])
    again = idx._encode(gpu_rotate(resid_d, idx.rotation), idx.codebooks).cpu().numpy()
    assert np.array_equal(again, codes)
    # encode_rows hands back what add_with_ids stored
    a2, codes2 = idx.encode_rows(X[:3000])
    order = np.argsort(ids_s)[:3000]
    assert np.array_equal(codes2, codes[order]) and np.array_equal(a2, ivfpq_ref.list_of_rows(off)[order])
    Q_d = dev(Q)
    for nprobe in (8, nlist):
        idx.nprobe = nprobe
        D, I, probes_d = search_and_probes(idx, Q, k)
        assert probes_d.shape == (Q.shape[0], nprobe)
        bias, lut, Qr = gpu_tables(idx, Q_d, probes_d)
        Do, Io = ivfpq_ref.scan(codes, off, ids_s, lut, probes_d.cpu().numpy(), bias, k)
        assert np.array_equal(D.view(np.uint32), Do.view(np.uint32)) and np.array_equal(I, Io), nprobe      # bit for bit
        # and the score is the inner product with the decoded row: q . c_l + (R q) . cw, in float64 up to the scan's rounding
        pos = np.argsort(ids_s)[np.searchsorted(np.sort(ids_s), I)]
        recon = c[ivfpq_ref.list_of_rows(off)[pos]].astype(np.float64) + ivfopq_ref.codewords(codes[pos.ravel()], cb).reshape(*pos.shape, d) @ R.astype(np.float64)
        want = np.einsum("qd,qkd->qk", Q.astype(np.float64), recon)
        assert np.abs(D - want).max() <= 2e-5
    # the rotation pays: the rotated codes are closer to the rows than plain PQ's of the same training
    rec = idx.reconstruct_batch(ids[:2000])
    plain = IVFPQIPIndex(d, nlist, m)
    plain.set_centroids(c)
    plain.codebooks = plain.train_codebooks(plain.training_residuals(dev(X)))
    plain.add_with_ids(X, ids)
    e_opq = ((rec - X[:2000]) ** 2).sum(axis=1).mean()
    e_pq = ((plain.reconstruct_batch(ids[:2000]) - X[:2000]) ** 2).sum(axis=1).mean()
    print(f"reconstruction error: opq {e_opq:.5f}, pq {e_pq:.5f}")
    assert e_opq < e_pq


@pytest.mark.parametrize("kind", [8, 16])
def test_refine_index_search_equals_the_restatements(kind):
    X, Q, ids = small_set()
    N, d, nlist, m, k = X.shape[0], X.shape[1], 100, 16, 10
    idx = IVFOPQRefineIPIndex(d, nlist, m, kind)
    assert isinstance(idx, IVFPQRefineIPIndex) and idx.k_factor == DEFAULT_K_FACTOR and (idx.opq_niter, idx.opq_niter_pq) == (50, 4)
    idx.opq_niter = 4
    idx.train(X)
    assert idx.search(Q, k)[1].max() == -1                                 # trained and empty: padding
    idx.add_with_ids(X[:9000], ids[:9000], chunk=4000)
    idx.search(Q, k)
    idx.add_with_ids(X[9000:], ids[9000:], chunk=4000)
    c, cb, codes, ids_s, off = idx.lists_host()
    rows, scales = idx.store_host()
    want_rows, want_scales = rr.quantise(X[(ids_s - 11) // 3], kind)       # the compact rows come from the UNROTATED rows
    assert np.array_equal(rows, want_rows) and (scales is None if kind == 16 else np.array_equal(scales, want_scales))
    store = N * d + N * 4 if kind == 8 else N * d * 2
    assert idx.hbm_bytes() == N * (m + 8) + (nlist + 1) * 8 + nlist * d * 4 + m * 256 * (d // m) * 4 + store + d * d * 4
    Q_d = dev(Q)
    for nprobe, k_factor in ((8, 5), (nlist, 50)):
        idx.nprobe, idx.k_factor = nprobe, k_factor
        kc = idx.candidates(k)
        D, I, probes_d = search_and_probes(idx, Q, k)
        bias, lut, _ = gpu_tables(idx, Q_d, probes_d)
        _, cand = ivfpq_ref.scan(codes, off, None, lut, probes_d.cpu().numpy(), bias, kc)
        Do, Io = rr.refine(rows, kind, scales, ids_s, Q, cand, k)           # re-ranked with the queries as they are
        assert np.array_equal(D.view(np.uint32), Do.view(np.uint32)) and np.array_equal(I, Io), (nprobe, k_factor)
    assert (I[:, 0] == ids[100:116]).all()
    rec = idx.reconstruct_batch(np.concatenate([ids[:500], [5, -7]]))       # unchanged: the stored row, dequantised
    pos = np.argsort(ids_s)[:500]
    assert np.array_equal(rec[:500].view(np.uint32), rr.dequantise(rows[pos], kind, None if scales is None else scales[pos]).view(np.uint32))
    assert np.isnan(rec[500:]).all()


@pytest.mark.parametrize("d,m", [(64, 16), (512, 64), (24, 4)])
def test_reconstruct_batch_within_the_chain_bound(d, m):
    N, nlist = 3000, 20
    rng = np.random.default_rng(d)
    idx = IVFOPQIPIndex(d, nlist, m)
    c, R = unit_rows(nlist, d, 3), orthonormal(d, 7)
    cb = (0.1 * rng.standard_normal((m, 256, d // m))).astype(np.float32)
    sizes = rng.multinomial(N, np.ones(nlist) / nlist)
    sizes[[2, 9]] += sizes[[3, 10]]
    sizes[[3, 10]] = 0                                                      # empty lists share offsets with their neighbours
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    codes = rng.integers(0, 256, (N, m)).astype(np.uint8)
    ids = rng.permutation(N).astype(np.int64) * 7 + 2
    idx.set_centroids(c)
    idx.set_codebooks(cb)
    idx.set_rotation(R)
    idx.adopt_lists(torch.from_numpy(codes), torch.from_numpy(ids), torch.from_numpy(off))
    ask = np.concatenate([ids[[0, N - 1]], ids[rng.permutation(N)[:300]], [1, -3, 7 * N + 9]])           # the last three: absent
    got = idx.reconstruct_batch(ask)
    again = idx.reconstruct_batch(ask)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    assert np.isnan(got[-3:]).all() and np.isfinite(got[:-3]).all()
    pos = np.argsort(ids)[np.searchsorted(np.sort(ids), ask[:-3])]
    cw = ivfopq_ref.codewords(codes[pos], cb)
    cl = c[ivfpq_ref.list_of_rows(off)[pos]].astype(np.float64)
    want = cl + cw @ R.astype(np.float64)                                   # c_l + R^T cw
    bound = gamma(d + 1, U32) * (np.abs(cl) + np.abs(cw) @ np.abs(R.astype(np.float64)))     # d fmaf steps and one addition
    err = np.abs(got[:-3].astype(np.float64) - want)
    print(f"decode d={d}: max err / bound {np.max(err / bound):.4f}")
    assert (err <= bound).all()


# --------------------------------------------------------------------------------------------------------------------- training
def test_training_quality_against_the_golden(golden_dir):
    """On the golden's data (ivfopq_ref.study_data: the restatement's own coarse quantizer installed, the restatement's training
    permutation) the GPU trainer at its defaults, judged by the float64 restatement on the GPU's rotation and codebooks."""
    gold = json.loads((golden_dir / "ivfopq_quality.json").read_text())
    p = ivfopq_ref.STUDY
    X, Q, c = ivfopq_ref.study_data()
    idx = IVFOPQIPIndex(p["d"], p["nlist"], p["m"])
    assert (idx.opq_niter, idx.opq_niter_pq, idx.niter, idx.seed) == (50, 4, 10, gold["seeds"][0])
    idx.set_centroids(c)
    resid_d = idx.training_residuals(dev(X))
    resid = resid_d.cpu().numpy()
    cb0 = idx.train_codebooks(resid_d).cpu().numpy()                        # iteration 0: R = I, today's PQ
    rot, cb = idx.train_rotation(resid_d)
    again = idx.train_rotation(resid_d)
    assert torch.equal(rot, again[0]) and torch.equal(cb, again[1])         # deterministic
    R, cbh = rot.cpu().numpy(), cb.cpu().numpy()
    ortho = np.abs(R.astype(np.float64) @ R.astype(np.float64).T - np.eye(p["d"])).max()
    e0 = ivfopq_ref.distortion(resid, np.eye(p["d"]), cb0)
    a = ivfopq_ref.distortion(resid, R, cbh)
    b = gold["distortion"][0]
    print(f"distortion: gpu iteration 0 {e0:.6e} (golden {gold['distortion_per_iteration'][0]:.6e}), gpu final {a:.6e}, "
          f"golden final {b:.6e}, margin {gold['distortion_margin']:.4e}, |RR^T - I| {ortho:.2e}")
    idx.rotation, idx.codebooks = rot, cb
    idx.add_with_ids(X, np.arange(p["n"], dtype=np.int64))
    idx.nprobe = p["nprobe"]
    _, I = idx.search(Q, p["k"])
    _, If = ip_topk_ref.ip_topk(X, Q, p["k"])
    rec = float(np.mean([len(set(I[q]) & set(If[q])) / p["k"] for q in range(Q.shape[0])]))
    print(f"recall@10: gpu {rec:.4f}, golden opq {gold['recall_at_10'][0]:.4f} (pq {gold['recall_at_10_pq']:.4f}), "
          f"allowance {gold['recall_allowance']:.4f}")
    assert a <= b * (1 + gold["distortion_margin"])
    assert a <= e0
    assert ortho <= 1e-5
    assert rec >= gold["recall_at_10"][0] - gold["recall_allowance"]


# --------------------------------------------------------------------------------------------------------------------- plugin
def test_search_index_builds_and_loads_the_opq_indexes(tmp_path):
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    from wise_amd.index import faiss_io
    from wise_amd.index.search_index_factory import SearchIndexFactory

    fdir, idir = tmp_path / "features", tmp_path / "index"
    fdir.mkdir()
    n, d = 3000, 512
    X = ivfpq_ref.clustered_unit_rows(n, d, 40, 0.3, 9)
    st = FeatureStoreFactory.create_store(FeatureStoreType.NUMPY, "video", str(fdir))
    st.enable_write(1000, 0)
    for i in range(n):
        st.add(i + 1, X[i:i + 1])
    st.close()
    si = SearchIndexFactory("video", "mlfoundations/open_clip/ViT-B-32/seeded-0", {"features_dir": fdir, "index_dir": idir})
    Qs = unit_rows(8, d, 3) * 0.1 + X[:8]
    nlist = reference_nlist(n)
    sample = np.sort(np.random.default_rng(1234).permutation(n)[:min(n, 100 * nlist)])
    for itype, cls, args in (("IndexIVFOPQ16", IVFOPQIPIndex, ()), ("IndexIVFOPQ16R8", IVFOPQRefineIPIndex, (8,))):
        si.create_index(itype)
        fn = si.get_index_filename(itype)
        assert fn.name == f"video-{itype}.faiss" and fn.exists() and faiss_io.index_fourcc(fn) == "WiOP"
        assert fn.stat().st_size < n * d * 4 // 2 + (n * (d + 4) if args else 0)      # codes, R (and int8 rows), not fp32 rows
        assert si.load_index(itype) is True and si.is_index_loaded()
        index = si.index
        assert type(index) is cls and index.m == 16 and index.nlist == nlist and index.ntotal == n
        # the in-memory index, built the way create_index builds it (the build is deterministic)
        built = cls(d, nlist, 16, *args)
        built.train(X[sample])
        built.add_with_ids(X, np.arange(n, dtype=np.int64) + 1)
        assert torch.equal(built.rotation, index.rotation)
        for a, b in zip(built.lists_host(), index.lists_host()):
            assert np.array_equal(a, b)
        index.parallel_mode = 1                                             # routes.py:899-902
        index.make_direct_map(True)
        for nprobe in (4, 1024):
            index.nprobe = built.nprobe = nprobe
            D, I = index.search(Qs, 5)
            Db, Ib = built.search(Qs, 5)
            assert np.array_equal(D.view(np.uint32), Db.view(np.uint32)) and np.array_equal(I, Ib)
        assert (I[:, 0] == np.arange(8) + 1).all() and (np.diff(D, axis=1) <= 0).all()      # a row finds itself
        rec, recb = index.reconstruct_batch([1, 17, 3000, 4000]), built.reconstruct_batch([1, 17, 3000, 4000])
        assert np.array_equal(rec, recb, equal_nan=True) and np.isnan(rec[3]).all()
        assert ((rec[:3] - X[[0, 16, 2999]]) ** 2).sum(axis=1).max() < 0.5
        dist, ids = si.search("video", "dog", topk=5)
        assert dist.shape == (5,) and ids.shape == (5,) and (ids >= 1).all()

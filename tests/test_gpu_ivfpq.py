"""-m gpu: IndexIVFPQ — the wise_pq_* / wise_ivfpq_scan kernels through the C ABI against the numpy restatement
(tests/ivfpq_ref.py), then the index and the SearchIndexFactory path on top of them."""
import json

import numpy as np
import pytest
import torch

import ivfpq_ref
from oracle import ip_topk_ref
from wise_amd import _lib
from wise_amd.index.ivf_flat import reference_nlist
from wise_amd.index.ivf_pq import IVFPQIPIndex

pytestmark = pytest.mark.gpu

TOL = 2e-5      # the project's search tolerance


def unit_rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_against(D, I, Do, Io, tol=TOL):
    assert D.shape == Do.shape and I.dtype == np.int64
    assert np.allclose(D, Do, atol=tol)
    gap_ok = np.ones_like(Io, dtype=bool)
    gap_ok[:, 1:] &= (Do[:, :-1] - Do[:, 1:]) > tol
    gap_ok[:, :-1] &= (Do[:, :-1] - Do[:, 1:]) > tol
    assert np.array_equal(I[gap_ok], Io[gap_ok])


def gpu_scan(codes, list_off, ids, lut, probes, bias, k):
    lib = _lib.lib()
    nq, m = lut.shape[0], lut.shape[1]
    nprobe, nlist = probes.shape[1], len(list_off) - 1
    need = lib.wise_ivfpq_scan_workspace_bytes(nq, nprobe, k, m)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    c_d, o_d, i_d, l_d, p_d, b_d = dev(codes), dev(list_off), dev(ids), dev(lut), dev(probes), dev(bias)
    D = torch.empty(nq, k, dtype=torch.float32, device="cuda")
    I = torch.empty(nq, k, dtype=torch.int64, device="cuda")
    rc = lib.wise_ivfpq_scan(c_d.data_ptr(), codes.shape[0], m, o_d.data_ptr(), nlist, i_d.data_ptr(), l_d.data_ptr(), nq,
                             p_d.data_ptr(), b_d.data_ptr(), nprobe, k, D.data_ptr(), I.data_ptr(), ws.data_ptr(), ws.numel(),
                             _lib.stream_ptr())
    _lib.check(rc, "wise_ivfpq_scan")
    torch.cuda.synchronize()
    return D.cpu().numpy(), I.cpu().numpy()


def scan_case(m, nlist=48, seed=0):
    """Lists of 0 .. ~400 rows (some empty), a tenth of the rows exact copies of their list's first row (exact ties)."""
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


@pytest.mark.parametrize("k", [1, 10, 100, 1000])
@pytest.mark.parametrize("m", [8, 16, 64, 128])
def test_scan_is_bit_equal_to_the_restatement(m, k):
    codes, list_off, ids = scan_case(m)
    nlist = len(list_off) - 1
    rng = np.random.default_rng(100 + m + k)
    for nq in (1, 3, 64):
        lut = (rng.standard_normal((nq, m, 256)) / np.sqrt(m)).astype(np.float32)
        for nprobe in (1, 8, 1024):
            probes = np.full((nq, nprobe), -1, dtype=np.int64)
            for q in range(nq):
                probes[q, :min(nprobe, nlist)] = rng.permutation(nlist)[:nprobe]
            if nprobe > 1:
                probes[rng.random(probes.shape) < 0.1] = -1
            bias = rng.standard_normal((nq, nprobe)).astype(np.float32)
            D, I = gpu_scan(codes, list_off, ids, lut, probes, bias, k)
            Do, Io = ivfpq_ref.scan(codes, list_off, ids, lut, probes, bias, k)
            what = f"m={m} k={k} nq={nq} nprobe={nprobe}"
            assert np.array_equal(D.view(np.uint32), Do.view(np.uint32)), what      # bit for bit
            assert np.array_equal(I, Io), what                                       # ties: the lower position wins
            if k == 1000 and nprobe == 1:
                assert (I[:, -1] == -1).all() and (D[:, -1] < -3e38).all()           # fewer rows than k: padding


def test_scan_refuses_what_it_does_not_serve():
    lib = _lib.lib()
    assert lib.wise_ivfpq_scan_workspace_bytes(1, 8, 10, 129) == 0
    assert lib.wise_ivfpq_scan_workspace_bytes(1, 8, 2049, 64) == 0
    assert lib.wise_ivfpq_scan_workspace_bytes(1, 2049, 10, 64) == 0
    assert lib.wise_ivfpq_scan_workspace_bytes(1, 2048, 2048, 128) > 0
    x = torch.zeros(256, dtype=torch.float32, device="cuda")
    assert lib.wise_pq_lut(x.data_ptr(), x.data_ptr(), 1, 64, 7, x.data_ptr(), 0) == -3      # WISE_E_UNSUPPORTED: d % m
    assert lib.wise_pq_lut(x.data_ptr(), x.data_ptr(), 1, 768, 4, x.data_ptr(), 0) == -3     # dsub = 192 > 96
    with pytest.raises(ValueError):
        IVFPQIPIndex(512, 10, 64, nbits=16)
    with pytest.raises(ValueError):
        IVFPQIPIndex(768, 10, 192)
    with pytest.raises(ValueError):
        IVFPQIPIndex(512, 10, 7)


@pytest.mark.parametrize("d,m", [(64, 16), (512, 64), (768, 8), (24, 4)])
def test_lut_and_bias_within_the_chain_bound(d, m):
    lib = _lib.lib()
    nq, nlist, nprobe, dsub = 5, 30, 7, d // m
    rng = np.random.default_rng(d + m)
    Q, c = unit_rows(nq, d, 1), unit_rows(nlist, d, 2)
    cb = (0.2 * rng.standard_normal((m, 256, dsub))).astype(np.float32)
    probes = np.stack([rng.permutation(nlist)[:nprobe] for _ in range(nq)]).astype(np.int64)
    probes[0, 1] = -1
    lut = torch.empty(nq, m, 256, dtype=torch.float32, device="cuda")
    bias = torch.empty(nq, nprobe, dtype=torch.float32, device="cuda")
    Qd, cd, cbd, pd = dev(Q), dev(c), dev(cb), dev(probes)
    _lib.check(lib.wise_pq_lut(Qd.data_ptr(), cbd.data_ptr(), nq, d, m, lut.data_ptr(), _lib.stream_ptr()), "wise_pq_lut")
    _lib.check(lib.wise_pq_bias(Qd.data_ptr(), cd.data_ptr(), pd.data_ptr(), nq, nprobe, nlist, d, bias.data_ptr(),
                                _lib.stream_ptr()), "wise_pq_bias")
    want = ivfpq_ref.lut(Q, cb)
    qn = np.linalg.norm(Q.astype(np.float64).reshape(nq, m, dsub), axis=2)              # [nq, m]
    cn = np.linalg.norm(cb.astype(np.float64), axis=2)                                  # [m, 256]
    bound = dsub * 2.0 ** -23 * qn[:, :, None] * cn[None]
    err = np.abs(lut.cpu().numpy().astype(np.float64) - want)
    print(f"lut: max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()
    wb = np.take_along_axis(Q.astype(np.float64) @ c.astype(np.float64).T, np.maximum(probes, 0), axis=1)
    wb[probes < 0] = 0.0
    bb = d * 2.0 ** -23 * np.linalg.norm(Q.astype(np.float64), axis=1)[:, None] * \
        np.linalg.norm(c.astype(np.float64), axis=1)[np.maximum(probes, 0)]
    errb = np.abs(bias.cpu().numpy().astype(np.float64) - wb)
    print(f"bias: max err {errb.max():.3e}")
    assert (errb <= bb).all()


def encode_data():
    """The issue's data: 20,000 seeded rows around 140 unit centres, noise 0.3 / sqrt(d), d = 64, m = 16, three Lloyd steps."""
    N, d, m = 20000, 64, 16
    X, c = ivfpq_ref.clustered_unit_rows(N, d, 140, 0.3, 21, return_centres=True)
    resid = (X - c[(X @ c.T).argmax(axis=1)]).astype(np.float32)
    cb = ivfpq_ref.train(resid, m, niter=3).astype(np.float32)
    return resid, cb, d, m


def gpu_encode(resid, cb, d, m):
    codes = torch.empty(resid.shape[0], m, dtype=torch.uint8, device="cuda")
    rd, cbd = dev(resid), dev(cb)
    _lib.check(_lib.lib().wise_pq_encode(rd.data_ptr(), cbd.data_ptr(), resid.shape[0], d, m, codes.data_ptr(), _lib.stream_ptr()),
               "wise_pq_encode")
    return codes.cpu().numpy()


def test_encode_equals_float64_off_near_ties():
    resid, cb, d, m = encode_data()
    dsub = d // m
    got = gpu_encode(resid, cb, d, m)
    s = ivfpq_ref.sub_scores(resid, cb)                                  # [n, m, 256] float64
    want = s.argmax(axis=2)
    top2 = np.partition(s, 254, axis=2)[:, :, 254:]
    gap = top2[:, :, 1] - top2[:, :, 0]
    rn = np.linalg.norm(resid.astype(np.float64).reshape(-1, m, dsub), axis=2)           # [n, m]
    cmax = np.linalg.norm(cb.astype(np.float64), axis=2).max(axis=1)                     # [m]
    eps = (dsub + 2) * 2.0 ** -23 * (rn * cmax[None] + 0.5 * cmax[None] ** 2)
    excused = gap <= 2 * eps
    mism = got != want
    print(f"encode: excused {excused.mean():.4%}, mismatches {mism.sum()}, unexcused {int((mism & ~excused).sum())}")
    assert excused.mean() <= 0.01
    assert not (mism & ~excused).any()


def test_update_is_a_sequential_fp32_mean_and_deterministic():
    lib = _lib.lib()
    resid, cb, d, m = encode_data()
    dsub = d // m
    codes = ivfpq_ref.encode(resid, cb)
    codes[codes[:, 0] == 255, 0] = 254                                  # codeword 255 of sub-space 0: empty
    rd, cd, cbd = dev(resid), dev(codes), dev(cb)
    outs = []
    for _ in range(2):
        out = torch.full_like(cbd, float("nan"))
        _lib.check(lib.wise_pq_update(rd.data_ptr(), cd.data_ptr(), resid.shape[0], d, m, cbd.data_ptr(), out.data_ptr(),
                                      _lib.stream_ptr()), "wise_pq_update")
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))              # the same bits run after run
    want, counts = ivfpq_ref.lloyd_update(resid, codes, cb)
    assert counts[0, 255] == 0 and np.array_equal(outs[0][0, 255], cb[0, 255])           # an empty codeword is unchanged
    r = np.abs(resid.astype(np.float64)).reshape(-1, m, dsub)
    rmax = np.zeros((m, 256))
    for j in range(m):
        np.maximum.at(rmax[j], codes[:, j], r[:, j].max(axis=1))
    bound = ((counts + 2) * 2.0 ** -24 * rmax)[:, :, None]
    err = np.abs(outs[0].astype(np.float64) - want)
    print(f"update: max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()


def test_decode_is_bit_equal():
    lib = _lib.lib()
    d, m, nlist = 64, 16, 20
    codes, list_off, _ = scan_case(m, nlist=nlist, seed=5)
    N = codes.shape[0]
    rng = np.random.default_rng(1)
    c = unit_rows(nlist, d, 3)
    cb = (0.1 * rng.standard_normal((m, 256, d // m))).astype(np.float32)
    pos = np.concatenate([rng.permutation(N)[:200], [0, N - 1, -1, N]]).astype(np.int64)
    out = torch.empty(len(pos), d, dtype=torch.float32, device="cuda")
    cd, pd, od, cend, cbd = dev(codes), dev(pos), dev(list_off), dev(c), dev(cb)
    _lib.check(lib.wise_pq_decode(cd.data_ptr(), N, pd.data_ptr(), len(pos), od.data_ptr(), nlist, cend.data_ptr(), cbd.data_ptr(),
                                  d, m, out.data_ptr(), _lib.stream_ptr()), "wise_pq_decode")
    got = out.cpu().numpy()
    ok = pos[:-2]
    want = ivfpq_ref.decode(codes[ok], ivfpq_ref.list_of_rows(list_off)[ok], c, cb, dtype=np.float32)
    assert np.array_equal(got[:-2].view(np.uint32), want.view(np.uint32))
    assert np.isnan(got[-2:]).all()


def test_index_search_equals_the_restatement_on_its_own_state():
    N, d, nlist, m, k = 20000, 64, 100, 16, 10
    X = ivfpq_ref.clustered_unit_rows(N, d, 140, 0.3, 31)
    Q = unit_rows(16, d, 4) * 0.2 + X[100:116]
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    ids = np.arange(N, dtype=np.int64) * 3 + 11
    idx = IVFPQIPIndex(d, nlist, m)
    with pytest.raises(RuntimeError):
        idx.add_with_ids(X, ids)
    idx.train(X)
    for s in range(0, N, 7000):
        idx.add_with_ids(X[s:s + 7000], ids[s:s + 7000])
    assert idx.ntotal == N and idx.is_trained
    c, cb, codes, ids_s, off = idx.lists_host()
    assert codes.shape == (N, m) and codes.dtype == np.uint8 and off[-1] == N and sorted(ids_s.tolist()) == ids.tolist()
    assert idx.hbm_bytes() == N * (m + 8) + (nlist + 1) * 8 + nlist * d * 4 + m * 256 * (d // m) * 4     # and no fp32 rows
    for nprobe in (8, nlist):
        idx.nprobe = nprobe
        D, I = idx.search(Q, k)
        probes = idx.probes_device(dev(Q), nprobe).cpu().numpy()
        bias = np.take_along_axis(Q.astype(np.float64) @ c.astype(np.float64).T, np.maximum(probes, 0), axis=1).astype(np.float32)
        Do, Io = ivfpq_ref.scan(codes, off, ids_s, ivfpq_ref.lut(Q, cb).astype(np.float32), probes, bias, k)
        check_against(D, I, Do, Io)
    # decoded rows are closer to the originals than the bare centroids are
    rec = idx.reconstruct_batch(ids[:500])
    a = (X[:500] @ c.T).argmax(axis=1)
    assert ((rec - X[:500]) ** 2).sum(axis=1).mean() < 0.5 * ((c[a] - X[:500]) ** 2).sum(axis=1).mean()


def test_search_index_builds_and_loads_an_ivfpq_index(tmp_path):
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    from wise_amd.index import faiss_io
    from wise_amd.index.search_index_factory import SearchIndexFactory

    fdir, idir = tmp_path / "features", tmp_path / "index"
    fdir.mkdir()
    X = ivfpq_ref.clustered_unit_rows(3000, 512, 40, 0.3, 9)
    st = FeatureStoreFactory.create_store(FeatureStoreType.WEBDATASET, "video", str(fdir))
    st.enable_write(2048, 20 * 1024 * 1024)
    for i in range(X.shape[0]):
        st.add(i + 1, X[i:i + 1])
    st.close()
    si = SearchIndexFactory("video", "mlfoundations/open_clip/ViT-B-32/seeded-0", {"features_dir": fdir, "index_dir": idir})
    assert not si.is_index_loaded()
    si.create_index("IndexIVFPQ16")
    fn = si.get_index_filename("IndexIVFPQ16")
    assert fn.name == "video-IndexIVFPQ16.faiss" and fn.exists() and faiss_io.index_fourcc(fn) == "IwPQ"
    assert fn.stat().st_size < 3000 * 512 * 4 // 2                      # codes, not rows
    assert si.load_index("IndexIVFPQ16") is True and si.is_index_loaded()
    index = si.index
    assert isinstance(index, IVFPQIPIndex) and index.m == 16 and index.nlist == reference_nlist(3000) and index.ntotal == 3000
    index.parallel_mode = 1                                             # routes.py:899-902
    index.nprobe = 1024
    index.make_direct_map(True)
    assert index.direct_map.type != index.direct_map.NoMap
    D, I = index.search(X[:8], 5)
    assert (I[:, 0] == np.arange(8) + 1).all() and (np.diff(D, axis=1) <= 0).all()      # a row finds itself
    rec = index.reconstruct_batch([1, 17, 3000])
    assert rec.shape == (3, 512) and ((rec - X[[0, 16, 2999]]) ** 2).sum(axis=1).max() < 0.5
    dist, ids = si.search("video", "dog", topk=5)
    assert dist.shape == (5,) and ids.shape == (5,) and (ids >= 1).all()


def test_training_quality_against_the_restatement(golden_dir):
    """(a) the GPU trainer's distortion on its training residuals <= (b) the float64 restatement's from the SAME initial
    codewords, times (1 + margin); margin and the recall allowance are the restatement's own five-seed spread, recorded in
    tests/golden/ivfpq_quality.json (computed on the CPU on this data)."""
    gold = json.loads((golden_dir / "ivfpq_quality.json").read_text())
    N, d, m, k, nprobe = 100000, 64, 16, 10, 32
    nlist = reference_nlist(N)
    X = ivfpq_ref.clustered_unit_rows(N, d, 300, 0.35, 11)
    Q = X[:64] + 0.05 * ivfpq_ref.clustered_unit_rows(64, d, 64, 1.0, 12)
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    idx = IVFPQIPIndex(d, nlist, m)
    sample = np.sort(np.random.default_rng(1234).permutation(N)[:min(N, 100 * nlist)])
    idx.train(X[sample])
    resid_d = idx.training_residuals(dev(X[sample]))
    resid = resid_d.cpu().numpy()
    init = idx.initial_codebooks(resid_d).cpu().numpy()
    assert np.array_equal(init, ivfpq_ref.initial_codebooks(resid, m))
    cb_gpu = idx.codebooks.cpu().numpy()
    cb_ref = ivfpq_ref.train(resid, m, niter=idx.niter, init=init)
    e0, a, b = ivfpq_ref.distortion(resid, init), ivfpq_ref.distortion(resid, cb_gpu), ivfpq_ref.distortion(resid, cb_ref)
    print(f"distortion: initial {e0:.6e}, gpu {a:.6e}, restatement {b:.6e}, margin {gold['distortion_margin']:.4e}")
    assert a <= b * (1 + gold["distortion_margin"])
    assert a <= e0                                                      # Lloyd never increases distortion
    # recall@10 at nprobe = 32 against the flat answer: the GPU index, and the restatement's codebooks on the same lists
    idx.add_with_ids(X, np.arange(N, dtype=np.int64))
    idx.nprobe = nprobe
    _, I = idx.search(Q, k)
    _, If = ip_topk_ref.ip_topk(X, Q, k)
    c, _, _, ids_s, off = idx.lists_host()
    Xs = X[ids_s]
    codes_ref = ivfpq_ref.encode(Xs - c[ivfpq_ref.list_of_rows(off)], cb_ref.astype(np.float32))
    probes = idx.probes_device(dev(Q), nprobe).cpu().numpy()
    bias = np.take_along_axis(Q.astype(np.float64) @ c.astype(np.float64).T, probes, axis=1).astype(np.float32)
    _, Ir = ivfpq_ref.scan(codes_ref, off, ids_s, ivfpq_ref.lut(Q, cb_ref.astype(np.float32)).astype(np.float32), probes, bias, k)
    rec_gpu = np.mean([len(set(I[q]) & set(If[q])) / k for q in range(64)])
    rec_ref = np.mean([len(set(Ir[q]) & set(If[q])) / k for q in range(64)])
    print(f"recall@10: gpu {rec_gpu:.4f}, restatement {rec_ref:.4f}, spread {gold['recall_spread']:.4f}")
    assert rec_gpu >= rec_ref - gold["recall_spread"]

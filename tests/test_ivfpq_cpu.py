"""IndexIVFPQ without a GPU: the numpy restatement (tests/ivfpq_ref.py) against brute force and against the flat oracle, the
'IwPQ' file round trip, and the index-type names create_index accepts."""
import numpy as np
import pytest

import ivfpq_ref
from oracle import ip_topk_ref
from wise_amd.index import faiss_io
from wise_amd.index.feature_search_index import parse_ivfpq_type

TOL = 2e-5      # the project's search tolerance


def unit_rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def check_against(D, I, Do, Io, tol=TOL):
    assert D.shape == Do.shape and I.dtype == np.int64
    assert np.allclose(D, Do, atol=tol)
    gap_ok = np.ones_like(Io, dtype=bool)
    gap_ok[:, 1:] &= (Do[:, :-1] - Do[:, 1:]) > tol
    gap_ok[:, :-1] &= (Do[:, :-1] - Do[:, 1:]) > tol
    assert np.array_equal(I[gap_ok], Io[gap_ok])


def small_index(N=3000, d=32, m=8, nlist=20, seed=0):
    """(centroids, codebooks f32, codes, ids, list_off) of a small clustered set, built by the restatement."""
    rng = np.random.default_rng(seed)
    c = unit_rows(nlist, d, seed + 1)
    X = c[rng.integers(0, nlist, N)] + 0.3 * unit_rows(N, d, seed + 2)
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    a = (X @ c.T).argmax(axis=1)
    order = np.argsort(a, kind="stable")
    X, a = X[order], a[order]
    list_off = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=nlist))]).astype(np.int64)
    resid = X - c[a]
    cb = ivfpq_ref.train(resid, m, niter=2).astype(np.float32)
    return c, cb, ivfpq_ref.encode(resid, cb), np.arange(N, dtype=np.int64) * 3 + 7, list_off


def test_scan_restatement_equals_decoded_brute_force():
    c, cb, codes, ids, list_off = small_index()
    nlist, k = c.shape[0], 25
    Q = unit_rows(6, c.shape[1], 9)
    rng = np.random.default_rng(3)
    probes = np.stack([rng.permutation(nlist)[:7] for _ in range(Q.shape[0])]).astype(np.int64)
    probes[1, 2] = -1
    lut = ivfpq_ref.lut(Q, cb).astype(np.float32)
    coarse = Q.astype(np.float64) @ c.astype(np.float64).T
    bias = np.take_along_axis(coarse, np.maximum(probes, 0), axis=1).astype(np.float32)
    D, I = ivfpq_ref.scan(codes, list_off, ids, lut, probes, bias, k)
    # brute force: decode every probed row, float64 dot products
    recon = ivfpq_ref.decode(codes, ivfpq_ref.list_of_rows(list_off), c, cb, dtype=np.float64)
    Do = np.full((Q.shape[0], k), ivfpq_ref.NEG, dtype=np.float32)
    Io = np.full((Q.shape[0], k), -1, dtype=np.int64)
    for q in range(Q.shape[0]):
        rows = np.concatenate([np.arange(list_off[l], list_off[l + 1]) for l in probes[q] if l >= 0])
        s = recon[rows] @ Q[q].astype(np.float64)
        o = np.lexsort((rows, -s))[:k]
        Do[q, :len(o)], Io[q, :len(o)] = s[o], ids[rows[o]]
    check_against(D, I, Do, Io)


def test_lossless_codebooks_reproduce_the_flat_answer():
    N, d, m, nlist, k = 2000, 32, 8, 12, 10
    rng = np.random.default_rng(5)
    c = unit_rows(nlist, d, 1)
    cb = (0.1 * rng.standard_normal((m, 256, d // m))).astype(np.float32)
    a = np.sort(rng.integers(0, nlist, N))
    list_off = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=nlist))]).astype(np.int64)
    want = rng.integers(0, 256, (N, m)).astype(np.uint8)
    X = ivfpq_ref.decode(want, a, c, cb, dtype=np.float32)      # every residual sub-vector IS a codeword
    codes = ivfpq_ref.encode(X - c[a], cb)
    assert np.array_equal(codes, want)
    ids = np.arange(N, dtype=np.int64) + 100
    Q = unit_rows(5, d, 2)
    probes = np.tile(np.arange(nlist, dtype=np.int64), (Q.shape[0], 1))
    bias = (Q.astype(np.float64) @ c.astype(np.float64).T).astype(np.float32)
    D, I = ivfpq_ref.scan(codes, list_off, ids, ivfpq_ref.lut(Q, cb).astype(np.float32), probes, bias, k)
    Df, If = ip_topk_ref.ip_topk(X, Q, k, ids=ids)
    check_against(D, I, Df, If)


def test_scan_restatement_ties_padding_and_empty_lists():
    m, k = 4, 6
    codes = np.array([[1, 2, 3, 4], [9, 9, 9, 9], [1, 2, 3, 4], [1, 2, 3, 4]], dtype=np.uint8)
    list_off = np.array([0, 2, 2, 4], dtype=np.int64)             # list 1 is empty
    lut = np.random.default_rng(0).standard_normal((1, m, 256)).astype(np.float32)
    probes = np.array([[2, 1, 0, -1]], dtype=np.int64)
    bias = np.zeros((1, 4), dtype=np.float32)
    D, I = ivfpq_ref.scan(codes, list_off, None, lut, probes, bias, k)
    tied = [i for i in I[0] if i in (0, 2, 3)]
    assert tied == [0, 2, 3]                                     # equal scores: the lower position first
    assert (I[0, 4:] == -1).all() and (D[0, 4:] == ivfpq_ref.NEG).all()


def test_ivf_pq_file_round_trip(tmp_path):
    c, cb, codes, ids, list_off = small_index(N=500, d=16, m=4, nlist=9)
    fn = tmp_path / "video-IndexIVFPQ4.faiss"
    faiss_io.write_ivf_pq_ip(fn, c, cb, codes, ids, list_off, nprobe=17)
    assert faiss_io.index_fourcc(fn) == "IwPQ"
    f = faiss_io.read_ivf_pq_ip(fn)
    assert np.array_equal(f["centroids"], c) and np.array_equal(f["codebooks"], cb)
    assert f["codes"].dtype == np.uint8 and np.array_equal(f["codes"], codes)
    assert np.array_equal(f["ids"], ids) and np.array_equal(f["list_off"], list_off) and f["nprobe"] == 17
    with pytest.raises(RuntimeError):
        faiss_io.read_ivf_flat_ip(fn)
    with pytest.raises(RuntimeError):
        faiss_io.read_idmap_flat_ip(fn)
    # most lists empty: the sparse size table
    off2 = np.array([0] * 9 + [500], dtype=np.int64)
    faiss_io.write_ivf_pq_ip(fn, c, cb, codes, ids, off2)
    f = faiss_io.read_ivf_pq_ip(fn)
    assert np.array_equal(f["list_off"], off2) and np.array_equal(f["codes"], codes) and f["nprobe"] == 1
    flat = tmp_path / "video-IndexIVFFlat.faiss"
    faiss_io.write_ivf_flat_ip(flat, c, np.zeros((500, 16), np.float32), ids, list_off)
    with pytest.raises(RuntimeError):
        faiss_io.read_ivf_pq_ip(flat)


def test_index_type_names():
    assert parse_ivfpq_type("IndexIVFPQ64", 512) == 64
    assert parse_ivfpq_type("IndexIVFPQ", 512) == 128
    assert parse_ivfpq_type("IndexIVFPQ96", 768) == 96
    with pytest.raises(ValueError, match=r"m <= 128.*IndexIVFPQ<m>"):
        parse_ivfpq_type("IndexIVFPQ", 768)
    with pytest.raises(ValueError):
        parse_ivfpq_type("IndexIVFPQ7", 512)
    with pytest.raises(ValueError):
        parse_ivfpq_type("IndexIVFPQ192", 768)                   # m > 128: out of scope
    for other in ("IndexFlatIP", "IndexIVFFlat", "IndexHNSWFlat", "IndexIVFPQx", "IndexIVFPQ-4"):
        assert parse_ivfpq_type(other, 512) is None


def _store(tmp_path, d, n=12):
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    from wise_amd.index.search_index_factory import SearchIndexFactory

    fdir, idir = tmp_path / "features", tmp_path / "index"
    fdir.mkdir()
    X = unit_rows(n, d, 9)
    st = FeatureStoreFactory.create_store(FeatureStoreType.WEBDATASET, "video", str(fdir))
    st.enable_write(2048, 20 * 1024 * 1024)
    for i in range(n):
        st.add(i + 1, X[i:i + 1])
    st.close()
    return SearchIndexFactory("video", "mlfoundations/open_clip/ViT-B-32/seeded-0", {"features_dir": fdir, "index_dir": idir})


def test_create_index_refuses_bad_names_before_any_gpu_work(tmp_path):
    si = _store(tmp_path, 768)
    with pytest.raises(NotImplementedError, match="IndexFlatIP, IndexIVFFlat and IndexIVFPQ<m>"):
        si.create_index("IndexHNSWFlat")
    with pytest.raises(ValueError, match="IndexIVFPQ<m>"):
        si.create_index("IndexIVFPQ")                            # m = d / 4 = 192 at d = 768
    with pytest.raises(ValueError):
        si.create_index("IndexIVFPQ7")
    assert si.get_index_filename("IndexIVFPQ64").name == "video-IndexIVFPQ64.faiss"
    assert not si.get_index_filename("IndexIVFPQ").exists()

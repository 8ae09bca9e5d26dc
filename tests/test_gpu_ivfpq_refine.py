"""-m gpu: IndexIVFPQ<m>R8 / R16 — wise_ivf_refine through the C ABI against the numpy restatement (tests/ivfpq_refine_ref.py),
D bit for bit and I id for id, then the stores, the index and the SearchIndexFactory path on top of it."""
import numpy as np
import pytest
import torch

import ivfpq_ref
import ivfpq_refine_ref as rr
from wise_amd import _lib
from wise_amd.index.ivf_flat import reference_nlist
from wise_amd.index.ivf_pq import DEFAULT_K_FACTOR, IVFPQIPIndex, IVFPQRefineIPIndex

pytestmark = pytest.mark.gpu


def unit_rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_rows(rows):
    return dev(rows.view(np.int16) if rows.dtype == np.uint16 else rows)


def gpu_refine(rows_d, kind, scales_d, N, d, ids_d, Q_d, cand_d, k):
    nq, kc = cand_d.shape
    D = torch.empty(nq, k, dtype=torch.float32, device="cuda")
    I = torch.empty(nq, k, dtype=torch.int64, device="cuda")
    rc = _lib.lib().wise_ivf_refine(rows_d.data_ptr(), kind, _lib.ptr(scales_d), N, d, _lib.ptr(ids_d), Q_d.data_ptr(), nq,
                                    cand_d.data_ptr(), kc, k, D.data_ptr(), I.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "wise_ivf_refine")
    return D, I


def store_case(kind, d, N=5000):
    """N rows of mixed norms, a tenth of them exact copies of an earlier row (equal scores), ids a permutation."""
    rng = np.random.default_rng(1000 * kind + d)
    X = unit_rows(N, d, d + kind) * rng.uniform(0.5, 2.0, (N, 1)).astype(np.float32)
    dup = np.flatnonzero(rng.random(N) < 0.1)
    dup = dup[dup > 0]
    X[dup] = X[rng.integers(0, dup)]
    rows, scales = rr.quantise(X, kind)
    ids = rng.permutation(N).astype(np.int64) * 5 + 3
    return rows, scales, ids


def prefix(Dfull, Ifull, k):
    """The answer for k from the answer for kc (the restatement's k best are the first k of its kc best: tests/test_ivfpq_refine_cpu.py)"""
    nq, kc = Dfull.shape
    D = np.full((nq, k), rr.NEG, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    D[:, :min(k, kc)], I[:, :min(k, kc)] = Dfull[:, :k], Ifull[:, :k]
    return D, I


@pytest.mark.parametrize("d", [16, 128, 512, 768])
@pytest.mark.parametrize("kind", [8, 16])
def test_refine_is_bit_equal_to_the_restatement(kind, d):
    rows, scales, ids = store_case(kind, d)
    N = rows.shape[0]
    rows_d, scales_d, ids_d = dev_rows(rows), (dev(scales) if kind == 8 else None), dev(ids)
    rng = np.random.default_rng(7 * d + kind)
    for nq in (1, 3, 256):
        Q = unit_rows(nq, d, nq + d) * np.float32(1.3)
        Q_d = dev(Q)
        for kc in (1, 10, 100, 2048):
            cand = np.stack([rng.permutation(N)[:kc] for _ in range(nq)]).astype(np.int64)
            if kc > 1:
                cand[rng.random(cand.shape) < 0.1] = -1          # holes: fewer than kc valid candidates
                cand[0, 1] = N + 5                               # a position past the end is skipped too
            if nq > 1:
                cand[1] = -1                                     # a query without any candidate
            cand_d = dev(cand)
            for with_ids in (True, False):
                Dfull, Ifull = rr.refine(rows, kind, scales, ids if with_ids else None, Q, cand, kc)
                for k in sorted({1, 10, kc}):
                    D, I = gpu_refine(rows_d, kind, scales_d, N, d, ids_d if with_ids else None, Q_d, cand_d, k)
                    Do, Io = prefix(Dfull, Ifull, k)
                    what = f"kind={kind} d={d} nq={nq} kc={kc} k={k} ids={with_ids}"
                    assert np.array_equal(D.cpu().numpy().view(np.uint32), Do.view(np.uint32)), what      # bit for bit
                    assert np.array_equal(I.cpu().numpy(), Io), what                                       # ties: the lower position wins
                if kc == 2048:
                    assert (Ifull[:, -1] == -1).all()             # ~200 holes each: fewer than k = kc valid candidates, padding


def test_equal_rows_tie_by_position():
    d, N = 128, 300
    X = np.repeat(unit_rows(3, d, 1), 100, axis=0)                # three runs of 100 identical rows
    Q = unit_rows(2, d, 2)
    cand = np.stack([np.random.default_rng(q).permutation(N)[:256] for q in range(2)]).astype(np.int64)
    for kind in (8, 16):
        rows, scales = rr.quantise(X, kind)
        D, I = gpu_refine(dev_rows(rows), kind, dev(scales) if kind == 8 else None, N, d, None, dev(Q), dev(cand), 256)
        Do, Io = rr.refine(rows, kind, scales, None, Q, cand, 256)
        assert np.array_equal(D.cpu().numpy().view(np.uint32), Do.view(np.uint32)) and np.array_equal(I.cpu().numpy(), Io)
        assert len(np.unique(Do[0])) == 3                         # really ties


def test_refine_refuses_what_it_does_not_serve():
    lib = _lib.lib()
    x = torch.zeros(4096, dtype=torch.float32, device="cuda")
    c = torch.zeros(4096, dtype=torch.int64, device="cuda")
    p = x.data_ptr()

    def call(kind, d, kc, k):
        return lib.wise_ivf_refine(p, kind, p, 1, d, 0, p, 1, c.data_ptr(), kc, k, p, c.data_ptr(), 0)

    assert call(8, 24, 10, 10) == -3 and call(8, 8, 10, 10) == -3 and call(8, 1040, 10, 10) == -3      # WISE_E_UNSUPPORTED
    assert call(16, 20, 10, 10) == -3 and call(16, 1032, 10, 10) == -3 and call(4, 64, 10, 10) == -3
    assert call(8, 64, 2049, 10) == -3 and call(8, 64, 10, 2049) == -3 and call(8, 64, 0, 1) == -3
    assert call(8, 64, 10, 10) == 0 and call(16, 24, 10, 20) == 0
    assert lib.wise_ivf_refine_rows(p, 8, p, 1, 24, c.data_ptr(), 1, p, 0) == -3
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        IVFPQRefineIPIndex(24, 10, 6, 8)                          # the int8 builder takes d % 16 == 0
    with pytest.raises(ValueError):
        IVFPQRefineIPIndex(64, 10, 16, 4)
    with pytest.raises(ValueError):
        IVFPQRefineIPIndex(64, 10, 7, 8)


def test_refine_under_graph_capture():
    kind, d, nq, kc, k = 8, 128, 4, 100, 10
    rows, scales, ids = store_case(kind, d)
    N = rows.shape[0]
    Q = unit_rows(nq, d, 5)
    cand = np.stack([np.random.default_rng(q).permutation(N)[:kc] for q in range(nq)]).astype(np.int64)
    rows_d, scales_d, ids_d, Q_d, cand_d = dev_rows(rows), dev(scales), dev(ids), dev(Q), dev(cand)
    D0, I0 = gpu_refine(rows_d, kind, scales_d, N, d, ids_d, Q_d, cand_d, k)      # eager: also loads the kernel before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D, I = gpu_refine(rows_d, kind, scales_d, N, d, ids_d, Q_d, cand_d, k)
    D.zero_()
    I.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(D, D0) and torch.equal(I, I0)
    Q2 = unit_rows(nq, d, 6)
    Q_d.copy_(dev(Q2))                                             # the replay reads the buffers it captured
    g.replay()
    torch.cuda.synchronize()
    Do, Io = rr.refine(rows, kind, scales, ids, Q2, cand, k)
    assert np.array_equal(D.cpu().numpy().view(np.uint32), Do.view(np.uint32)) and np.array_equal(I.cpu().numpy(), Io)


def test_refine_operator_equals_the_c_abi():
    import wise_amd.torch_ops  # noqa: F401

    d, nq, kc, k = 128, 5, 64, 10
    for kind in (8, 16):
        rows, scales, ids = store_case(kind, d)
        N = rows.shape[0]
        Q_d = dev(unit_rows(nq, d, 8))
        cand_d = dev(np.stack([np.random.default_rng(q).permutation(N)[:kc] for q in range(nq)]).astype(np.int64))
        rows_d, scales_d, ids_d = dev_rows(rows), (dev(scales) if kind == 8 else None), dev(ids)
        D, I = torch.ops.wise_hip.ivf_refine(rows_d, scales_d, ids_d, Q_d, cand_d, k)
        D0, I0 = gpu_refine(rows_d, kind, scales_d, N, d, ids_d, Q_d, cand_d, k)
        assert torch.equal(D, D0) and torch.equal(I, I0)
    with pytest.raises(ValueError):
        torch.ops.wise_hip.ivf_refine(dev_rows(rr.quantise_i8(unit_rows(4, 16, 0))[0]), None, None, Q_d[:, :16].contiguous(), cand_d, k)


def gpu_tables(idx, Q_d, probes_d):
    """bias and lut as the index's own search computes them (wise_pq_bias / wise_pq_lut)"""
    lib, st = _lib.lib(), _lib.stream_ptr()
    nq, nprobe = probes_d.shape
    bias = torch.empty(nq, nprobe, dtype=torch.float32, device="cuda")
    _lib.check(lib.wise_pq_bias(Q_d.data_ptr(), idx.centroids.data_ptr(), probes_d.data_ptr(), nq, nprobe, idx.nlist, idx.d,
                                bias.data_ptr(), st), "wise_pq_bias")
    lut = torch.empty(nq, idx.m, 256, dtype=torch.float32, device="cuda")
    _lib.check(lib.wise_pq_lut(Q_d.data_ptr(), idx.codebooks.data_ptr(), nq, idx.d, idx.m, lut.data_ptr(), st), "wise_pq_lut")
    return bias.cpu().numpy(), lut.cpu().numpy()


@pytest.mark.parametrize("kind", [8, 16])
def test_index_stores_search_reconstruct_and_bytes(kind):
    N, d, nlist, m, k = 20000, 64, 100, 16, 10
    X = ivfpq_ref.clustered_unit_rows(N, d, 140, 0.3, 31)
    Q = unit_rows(16, d, 4) * 0.2 + X[100:116]
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    ids = np.arange(N, dtype=np.int64) * 3 + 11
    idx = IVFPQRefineIPIndex(d, nlist, m, kind)
    assert idx.k_factor == DEFAULT_K_FACTOR and isinstance(idx, IVFPQIPIndex)
    with pytest.raises(RuntimeError):
        idx.add_with_ids(X, ids)
    idx.train(X)
    assert idx.search(Q, k)[1].max() == -1                        # trained and empty: padding
    idx.add_with_ids(X[:9000], ids[:9000], chunk=4000)            # several chunks
    idx.search(Q, k)                                              # merges the lists
    idx.add_with_ids(X[9000:], ids[9000:], chunk=4000)            # into non-empty lists
    assert idx.ntotal == N
    c, cb, codes, ids_s, off = idx.lists_host()
    rows, scales = idx.store_host()
    Xs = X[(ids_s - 11) // 3]                                     # the rows in list order
    want_rows, want_scales = rr.quantise(Xs, kind)
    assert rows.dtype == want_rows.dtype and np.array_equal(rows, want_rows)
    assert scales is None if kind == 16 else np.array_equal(scales.view(np.uint32), want_scales.view(np.uint32))
    store = N * d + N * 4 if kind == 8 else N * d * 2
    assert idx.hbm_bytes() == N * (m + 8) + (nlist + 1) * 8 + nlist * d * 4 + m * 256 * (d // m) * 4 + store
    Q_d = dev(Q)
    for nprobe, k_factor in ((8, 5), (nlist, 50), (nlist, 1000)):
        idx.nprobe, idx.k_factor = nprobe, k_factor
        kc = idx.candidates(k)
        assert kc == min(k * k_factor, 2048)                      # clamped, not refused
        D, I = idx.search(Q, k)
        probes_d = idx.probes_device(Q_d, nprobe).contiguous()
        bias, lut = gpu_tables(idx, Q_d, probes_d)
        _, cand = ivfpq_ref.scan(codes, off, None, lut, probes_d.cpu().numpy(), bias, kc)
        Do, Io = rr.refine(rows, kind, scales, ids_s, Q, cand, k)
        assert np.array_equal(D.view(np.uint32), Do.view(np.uint32)) and np.array_equal(I, Io), (nprobe, k_factor)
    with pytest.raises(ValueError):
        idx.search(Q, 2049)
    # re-ranked by good rows a query finds the row it was made from, which the codes alone often miss
    assert (I[:, 0] == ids[100:116]).all()
    rec = idx.reconstruct_batch(np.concatenate([ids[:500], [5, -7]]))
    pos = np.argsort(ids_s)[:500]                                 # ids are ascending in X: position of ids[i]
    assert np.array_equal(rec[:500].view(np.uint32), rr.dequantise(rows[pos], kind, None if scales is None else scales[pos]).view(np.uint32))
    assert np.isnan(rec[500:]).all()                              # unknown ids


def test_search_index_builds_and_loads_a_refine_index(tmp_path):
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    from wise_amd.index import faiss_io
    from wise_amd.index.search_index_factory import SearchIndexFactory

    fdir, idir = tmp_path / "features", tmp_path / "index"
    fdir.mkdir()
    n, d = 3000, 512
    X = ivfpq_ref.clustered_unit_rows(n, d, 40, 0.3, 9)
    st = FeatureStoreFactory.create_store(FeatureStoreType.WEBDATASET, "video", str(fdir))
    st.enable_write(2048, 20 * 1024 * 1024)
    for i in range(n):
        st.add(i + 1, X[i:i + 1])
    st.close()
    si = SearchIndexFactory("video", "mlfoundations/open_clip/ViT-B-32/seeded-0", {"features_dir": fdir, "index_dir": idir})
    si.create_index("IndexIVFPQ16R8")
    fn = si.get_index_filename("IndexIVFPQ16R8")
    assert fn.name == "video-IndexIVFPQ16R8.faiss" and fn.exists() and faiss_io.index_fourcc(fn) == "WiPR"
    assert fn.stat().st_size < n * d * 4 // 2                           # codes and int8 rows, not fp32 rows
    assert si.load_index("IndexIVFPQ16R8") is True and si.is_index_loaded()
    index = si.index
    assert isinstance(index, IVFPQRefineIPIndex) and (index.m, index.kind, index.k_factor) == (16, 8, DEFAULT_K_FACTOR)
    assert index.nlist == reference_nlist(n) and index.ntotal == n
    # the index create_index built, built again the same way (the build is deterministic)
    built = IVFPQRefineIPIndex(d, reference_nlist(n), 16, 8)
    sample = np.sort(np.random.default_rng(1234).permutation(n)[:min(n, 100 * built.nlist)])
    built.train(X[sample])
    built.add_with_ids(X, np.arange(n, dtype=np.int64) + 1)
    for a, b in zip(built.lists_host() + built.store_host(), index.lists_host() + index.store_host()):
        assert np.array_equal(a, b)
    index.parallel_mode = 1                                             # routes.py:899-902
    index.make_direct_map(True)
    Qs = unit_rows(8, d, 3) * 0.1 + X[:8]
    for nprobe in (4, 1024):
        index.nprobe = built.nprobe = nprobe
        D, I = index.search(Qs, 5)
        Db, Ib = built.search(Qs, 5)
        assert np.array_equal(D.view(np.uint32), Db.view(np.uint32)) and np.array_equal(I, Ib)      # exactly as the built one
    assert (I[:, 0] == np.arange(8) + 1).all() and (np.diff(D, axis=1) <= 0).all()
    rec = index.reconstruct_batch([1, 17, 3000, 4000])
    assert rec.shape == (4, 512) and np.abs(rec[:3] - X[[0, 16, 2999]]).max() < 1 / 127 and np.isnan(rec[3]).all()
    dist, ids = si.search("video", "dog", topk=5)
    assert dist.shape == (5,) and ids.shape == (5,) and (ids >= 1).all()
    # the bf16 type goes the same way
    si.create_index("IndexIVFPQ16R16")
    si.load_index("IndexIVFPQ16R16")
    assert si.index.kind == 16 and si.index.ntotal == n and faiss_io.index_fourcc(si.get_index_filename("IndexIVFPQ16R16")) == "WiPR"
    si.index.nprobe = 1024
    assert (si.index.search(Qs, 5)[1][:, 0] == np.arange(8) + 1).all()

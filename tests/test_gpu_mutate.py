"""-m gpu: remove_ids on every index type and FeatureSearchIndex.update_index.  The contract: after a removal the index is,
byte for byte, the index with the same trained state that received only the kept rows in the same order — so every search,
filtered search, range_search and reconstruct_batch returns that index's bits."""
import os

import numpy as np
import pytest
import torch

import ivfpq_ref
from wise_amd.index import faiss_io
from wise_amd.index.flat_ip import FlatIPIndex
from wise_amd.index.ivf_flat import IVFFlatIPIndex
from wise_amd.index.ivf_pq import IVFOPQRefineIPIndex, IVFPQIPIndex, IVFPQRefineIPIndex
from wise_amd.index.ivf_sq import IVFSQIPIndex
from wise_amd.index.selector import IDSelectorBatch, IDSelectorNot, IDSelectorRange, SearchParameters, SearchParametersIVF

pytestmark = pytest.mark.gpu

N, D, NLIST, M = 4096, 64, 16, 16
KINDS = ["flat", "ivfflat", "sq8", "pq", "pqr8", "pqr16", "opqr8"]
RANGE_KINDS = ("flat", "ivfflat", "sq8")
SMALL_SCRATCH = 100 * 1024        # several chunks on every array of 4096 rows that is wider than 25 bytes


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def new_index(kind):
    return {"flat": lambda: FlatIPIndex(D), "ivfflat": lambda: IVFFlatIPIndex(D, NLIST), "sq8": lambda: IVFSQIPIndex(D, NLIST),
            "pq": lambda: IVFPQIPIndex(D, NLIST, M), "pqr8": lambda: IVFPQRefineIPIndex(D, NLIST, M, 8),
            "pqr16": lambda: IVFPQRefineIPIndex(D, NLIST, M, 16), "opqr8": lambda: IVFOPQRefineIPIndex(D, NLIST, M, 8)}[kind]()


_DATA = {}


def data():
    """rows, ids (a permutation of 3 N), queries — computed once"""
    if not _DATA:
        X = ivfpq_ref.clustered_unit_rows(N, D, 24, 0.35, 77)
        ids = np.random.default_rng(5).permutation(3 * N)[:N].astype(np.int64)
        Q = X[:8] + np.float32(0.05) * ivfpq_ref.clustered_unit_rows(8, D, 8, 0.5, 3)
        _DATA.update(X=X, ids=ids, Q=np.ascontiguousarray(Q, dtype=np.float32))
    return _DATA["X"], _DATA["ids"], _DATA["Q"]


_TRAINED = {}


def trained(kind):
    """The trained state of `kind`, trained once: what set_centroids / set_codebooks / set_rotation / set_trained take."""
    if kind not in _TRAINED:
        X, _, _ = data()
        idx = new_index(kind)
        state = {}
        if kind != "flat":
            if kind.startswith("opq"):
                idx.opq_niter = 3
            idx.train(X)
            state["centroids"] = idx.centroids.cpu().numpy()
            if hasattr(idx, "codebooks"):
                state["codebooks"] = idx.codebooks.cpu().numpy()
            if hasattr(idx, "rotation"):
                state["rotation"] = idx.rotation.cpu().numpy()
            if kind == "sq8":
                state["trained"] = idx.trained.cpu().numpy()
        _TRAINED[kind] = state
    return _TRAINED[kind]


def fresh(kind, rows, ids, step=1500):
    """An index of `kind` with the shared trained state that receives rows / ids in this order."""
    idx, state = new_index(kind), trained(kind)
    if "centroids" in state:
        idx.set_centroids(state["centroids"])
    if "codebooks" in state:
        idx.set_codebooks(state["codebooks"])
    if "rotation" in state:
        idx.set_rotation(state["rotation"])
    if "trained" in state:
        idx.set_trained(state["trained"][:D], state["trained"][D:])
    if hasattr(idx, "nprobe"):
        idx.nprobe = 4
    for s in range(0, len(rows), step):
        idx.add_with_ids(rows[s:s + step], ids[s:s + step])
    return idx


def host_state(idx):
    """Every per-row array and the offsets, as numpy"""
    if isinstance(idx, FlatIPIndex):
        idx._finalize()
        return [idx._X.cpu().numpy(), idx._ids.cpu().numpy()]
    out = list(idx.lists_host())
    if hasattr(idx, "store_host"):
        out += [a for a in idx.store_host() if a is not None]
    return out


def same_state(a, b):
    sa, sb = host_state(a), host_state(b)
    assert len(sa) == len(sb)
    for x, y in zip(sa, sb):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert a.ntotal == b.ntotal


def same_answers(kind, a, b, some_ids):
    _, _, Q = data()
    ivf = kind != "flat"
    for nq in (1, 8):
        q = torch.from_numpy(Q[:nq]).cuda()
        Da, Ia = a.search_device(q, 20)
        Db, Ib = b.search_device(q, 20)
        assert torch.equal(Da.view(torch.int32), Db.view(torch.int32)) and torch.equal(Ia, Ib), (kind, nq)
    sel = IDSelectorBatch(some_ids)
    params = SearchParametersIVF(sel=sel, nprobe=8) if ivf else SearchParameters(sel=sel)
    Da, Ia = a.search(Q, 20, params=params)
    Db, Ib = b.search(Q, 20, params=params)
    assert np.array_equal(bits(Da), bits(Db)) and np.array_equal(Ia, Ib), kind
    if kind in RANGE_KINDS:
        for p in (None, params):
            la, Da, Ia = a.range_search(Q, 0.55, params=p)
            lb, Db, Ib = b.range_search(Q, 0.55, params=p)
            assert la[-1] > 0 or p is not None
            assert np.array_equal(la, lb) and np.array_equal(bits(Da), bits(Db)) and np.array_equal(Ia, Ib), kind


def selectors(ids):
    rng = np.random.default_rng(11)
    third = rng.permutation(ids)[: N // 3]
    return {"batch": (IDSelectorBatch(np.concatenate([third, [-5, 10 ** 12]])), np.isin(ids, third)),
            "range": (IDSelectorRange(N, 2 * N), (ids >= N) & (ids < 2 * N)),
            "not_batch": (IDSelectorNot(IDSelectorBatch(third)), ~np.isin(ids, third))}


@pytest.mark.parametrize("sel_name", ["batch", "range", "not_batch"])
@pytest.mark.parametrize("kind", KINDS)
def test_remove_ids_leaves_the_index_of_the_kept_rows(kind, sel_name):
    X, ids, _ = data()
    sel, gone = selectors(ids)[sel_name]
    a = fresh(kind, X, ids)
    if kind != "flat":
        a.make_direct_map(True)                          # BEFORE the removal
    removed = a.remove_ids(sel, scratch_bytes=SMALL_SCRATCH)
    b = fresh(kind, X[~gone], ids[~gone])
    assert removed == int(gone.sum()) and a.ntotal == N - removed
    same_state(a, b)
    same_answers(kind, a, b, ids[::5])
    ask = np.concatenate([ids[gone][:6], ids[~gone][:6], [10 ** 12]])
    ra, rb = a.reconstruct_batch(ask), b.reconstruct_batch(ask)
    assert np.isnan(ra[:6]).all() and np.isnan(ra[-1]).all() and not np.isnan(ra[6:12]).any()
    assert np.array_equal(bits(ra), bits(rb))
    # again: nothing left to remove, nothing changes
    before = host_state(a)
    assert a.remove_ids(sel, scratch_bytes=SMALL_SCRATCH) == 0
    for x, y in zip(before, host_state(a)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


@pytest.mark.parametrize("kind", KINDS)
def test_edges_all_none_readd_pending(kind):
    X, ids, Q = data()
    sel, gone = selectors(ids)["batch"]
    # an array of ids is a selector; rows still pending are merged first; the default workspace
    a = fresh(kind, X, ids)
    assert a.remove_ids(ids[gone]) == int(gone.sum())
    same_state(a, fresh(kind, X[~gone], ids[~gone]))
    # re-adding the removed rows: the index that received kept-then-removed rows
    a.add_with_ids(X[gone], ids[gone])
    order = np.concatenate([np.flatnonzero(~gone), np.flatnonzero(gone)])
    c = fresh(kind, X[order], ids[order])
    same_state(a, c)
    same_answers(kind, a, c, ids[::7])
    # removing nothing leaves the bytes as they were
    before = host_state(a)
    assert a.remove_ids(IDSelectorBatch([-1, 10 ** 12])) == 0 and a.remove_ids(IDSelectorRange(5, 5)) == 0
    for x, y in zip(before, host_state(a)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    # removing everything leaves a searchable empty index that takes rows again
    assert a.remove_ids(IDSelectorRange(-1, 10 ** 15)) == N and a.ntotal == 0
    D_, I_ = a.search(Q, 5)
    assert (I_ == -1).all()
    assert a.remove_ids(ids[:10]) == 0
    a.add_with_ids(X, ids)
    same_state(a, fresh(kind, X, ids))


def test_slice_of_a_sharded_index_refuses():
    X, ids, _ = data()
    whole = fresh("sq8", X, ids)
    c, tr, codes, ids_s, off = whole.lists_host()
    part = IVFSQIPIndex(D, NLIST)
    part.set_centroids(c)
    part.set_trained(tr[:D], tr[D:])
    lo = 1000
    part.adopt_lists(torch.from_numpy(codes[lo:]), torch.from_numpy(ids_s[lo:]), torch.from_numpy(np.clip(off - lo, 0, N - lo)), pos_base=lo)
    with pytest.raises(NotImplementedError, match="pos_base"):
        part.remove_ids(ids[:5])
    assert part.ntotal == N - lo


def test_flat_reserved_capacity_and_implicit_ids():
    X, ids, _ = data()
    a = FlatIPIndex(D)
    a.reserve(N)
    a.add_with_ids(X, ids)
    store = a._store.reserved.data_ptr()
    gone = np.isin(ids, ids[100:900])
    assert a.remove_ids(ids[100:900], scratch_bytes=SMALL_SCRATCH) == 800
    assert a._store.reserved.data_ptr() == store and a._store.reserved.shape[0] == N and a._X.data_ptr() == store      # the capacity stays
    a.add_with_ids(X[100:500], ids[100:500])                                                 # ... and is filled from the new end
    assert a._X.data_ptr() == store and a.ntotal == N - 400
    order = np.concatenate([np.flatnonzero(~gone), np.arange(100, 500)])
    same_state(a, fresh("flat", X[order], ids[order]))
    # rows adopted with implicit ids (id_base + row) keep their ids when rows before them go
    b = FlatIPIndex(D).adopt(torch.from_numpy(X).cuda(), None, id_base=50)
    assert b.remove_ids(IDSelectorRange(50, 60)) == 10
    same_state(b, fresh("flat", X[10:], np.arange(60, 50 + N, dtype=np.int64)))


def test_flat_shadows_are_those_of_a_fresh_index():
    """Above 2^18 rows a single query goes through the reduced-precision shadow.  After a removal the two-stage path and
    the batched path return the bits of a fresh index over the kept rows, whichever shadows this box builds."""
    n, d = 300_000, 64
    X = ivfpq_ref.clustered_unit_rows(n, d, 200, 0.4, 8)
    ids = np.arange(n, dtype=np.int64) * 2 + 1
    Q = np.ascontiguousarray(X[1000:1008] + np.float32(0.02) * X[2000:2008], dtype=np.float32)
    a = FlatIPIndex(d)
    a.add_with_ids(X, ids)
    a.search(Q[:1], 10)                                  # the shadows exist now (if the box builds them)
    had = a._Xq is not None or a._Xb is not None
    gone = np.zeros(n, bool)
    gone[np.random.default_rng(1).permutation(n)[:20_000]] = True
    gone[1000:1004] = True                               # some of the queries' own rows
    counted = sum(a.shadow_counts())
    assert a.remove_ids(ids[gone]) == int(gone.sum()) and a.ntotal >= 1 << 18
    b = FlatIPIndex(d)
    b.add_with_ids(X[~gone], ids[~gone])
    for nq in (1, 8):
        Da, Ia = a.search(Q[:nq], 10)
        Db, Ib = b.search(Q[:nq], 10)
        assert np.array_equal(bits(Da), bits(Db)) and np.array_equal(Ia, Ib), nq
    assert not np.isin(Ia, ids[gone]).any()
    if had:                                              # rebuilt over the kept rows, and the counters went on counting
        for name in ("_Xq", "_scales8", "_norms8", "_Xb", "_norms"):
            ta, tb = getattr(a, name), getattr(b, name)
            assert (ta is None) == (tb is None), name
            if ta is not None:
                assert ta.shape == tb.shape and torch.equal(ta, tb), name
        assert sum(a.shadow_counts()) - counted == sum(b.shadow_counts()) > 0


def test_extra_memory_is_the_workspace_not_the_payload():
    """IVFFlat, 40,000 x 512 fp32 = 80 MB of rows, half of them removed through an 8 MiB scratch: the peak above what was
    allocated before the call stays under scratch + bitmap + plan + 4 MiB (the caching allocator's 2 MiB block rounding on
    two small tensors).  A second copy of the kept rows is 40 MB and fails this."""
    n, d, nlist = 40_000, 512, 16
    X = ivfpq_ref.clustered_unit_rows(n, d, 16, 0.4, 2)
    ids = np.random.default_rng(4).permutation(n).astype(np.int64)
    idx = IVFFlatIPIndex(d, nlist)
    idx.set_centroids(ivfpq_ref.clustered_unit_rows(nlist, d, nlist, 0.4, 6))
    idx.add_with_ids(X, ids)
    idx._finalize()
    sel = IDSelectorBatch(ids[ids % 2 == 0])
    scratch = 8 << 20
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    removed = idx.remove_ids(sel, scratch_bytes=scratch)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    bitmap, plan = (n + 31) // 32 * 4, ((n + 2047) // 2048 + 1) * 8
    print(f"remove_ids peak extra memory: {extra} bytes (scratch {scratch}, bitmap {bitmap}, plan {plan})")
    assert removed == n // 2
    assert extra < scratch + bitmap + plan + (4 << 20)
    keep = ids % 2 == 1
    b = IVFFlatIPIndex(d, nlist)
    b.set_centroids(idx.centroids.cpu().numpy())
    b.add_with_ids(X[keep], ids[keep])
    same_state(idx, b)


# ------------------------------------------------------------------------------------------------ the plugin
def write_shard(fdir, first_shard, ids, rows):
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    st = FeatureStoreFactory.create_store(FeatureStoreType.WEBDATASET, "video", str(fdir))
    st.enable_write(1024, 20 * 1024 * 1024, first_shard=first_shard)
    for i, r in zip(ids, rows):
        st.add(int(i), r[None, :])
    st.close()


PLUGIN_TYPES = ["IndexFlatIP", "IndexIVFFlat", "IndexIVFSQ8", "IndexIVFPQ16R8"]


@pytest.fixture(scope="module")
def plugin(tmp_path_factory):
    """A store of three shards of 1024 rows and the four index files built from it; then the store loses its middle shard and
    gains a fourth of 512 rows."""
    from wise_amd.index.search_index_factory import SearchIndexFactory
    root = tmp_path_factory.mktemp("mutate")
    fdir, idir = root / "features", root / "index"
    fdir.mkdir()
    n_old, n_new = 3072, 512
    X = ivfpq_ref.clustered_unit_rows(n_old + n_new, D, 24, 0.35, 21)
    ids = np.arange(1, n_old + n_new + 1, dtype=np.int64)
    write_shard(fdir, 0, ids[:n_old], X[:n_old])
    si = SearchIndexFactory("video", "mlfoundations/open_clip/ViT-B-32/seeded-0", {"features_dir": fdir, "index_dir": idir})
    for t in PLUGIN_TYPES:
        si.create_index(t)
    write_shard(fdir, 3, ids[n_old:], X[n_old:])
    os.remove(fdir / "video-000001.tar")
    kept = np.concatenate([np.arange(0, 1024), np.arange(2048, n_old)])
    return si, X, ids, kept, np.arange(n_old, n_old + n_new)


@pytest.mark.parametrize("index_type", PLUGIN_TYPES)
def test_update_index_brings_the_file_in_line_with_the_store(plugin, index_type, tmp_path):
    si, X, ids, kept, new = plugin
    fn = si.get_index_filename(index_type)
    # the index with the file's trained state that received the old kept rows, then the new rows
    if index_type == "IndexFlatIP":
        want = FlatIPIndex(D)
    elif index_type == "IndexIVFFlat":
        f = faiss_io.read_ivf_flat_ip(fn)
        want = IVFFlatIPIndex(D, f["centroids"].shape[0])
    elif index_type == "IndexIVFSQ8":
        f = faiss_io.read_ivf_sq_ip(fn)
        want = IVFSQIPIndex(D, f["centroids"].shape[0])
        want.set_trained(f["trained"][:D], f["trained"][D:])
    else:
        f = faiss_io.read_ivf_pq_refine_ip(fn)
        want = IVFPQRefineIPIndex(D, f["centroids"].shape[0], 16, 8, k_factor=f["k_factor"])
        want.set_codebooks(f["codebooks"])
    if index_type != "IndexFlatIP":
        assert f["ids"].shape[0] == 3072
        want.set_centroids(f["centroids"])
        want.nprobe = f["nprobe"]
    want.add_with_ids(X[kept], ids[kept])
    want.add_with_ids(X[new], ids[new])
    want_fn = tmp_path / "want.faiss"
    si._write_index_file(want, want_fn)
    assert si.update_index(index_type) == (512, 1024)
    assert fn.read_bytes() == want_fn.read_bytes()
    assert [p.name for p in fn.parent.iterdir() if ".tmp-" in p.name] == []
    assert not hasattr(si, "feature_extractor")          # update_index builds no extractor
    # a second update has nothing to do and leaves the file alone
    stamp = fn.stat().st_mtime_ns
    assert si.update_index(index_type) == (0, 0) and fn.stat().st_mtime_ns == stamp
    # load_index + search agree with that index
    assert si.load_index(index_type) is True and si.index.ntotal == 2048 + 512
    Q = np.ascontiguousarray(X[[5, 2100, 3100, 1500]], dtype=np.float32)      # the last one's row is gone
    if hasattr(si.index, "nprobe"):
        si.index.nprobe = want.nprobe = 8
    Da, Ia = si.index.search(Q, 10)
    Db, Ib = want.search(Q, 10)
    assert np.array_equal(bits(Da), bits(Db)) and np.array_equal(Ia, Ib)
    assert Ia[0, 0] == 6 and Ia[1, 0] == 2101 and Ia[2, 0] == 3101 and not np.isin(Ia, ids[1024:2048]).any()
    del si.index, si.feature_extractor

"""-m gpu: what FlatIPIndex and FlatSQfp16IPIndex share (wise_amd/index/flat_common.py), one body over both classes: the reserved
storage across a removal, the answers after it, adopt over a reservation, and rows_host through the plugin's table of exhaustive types.
The rows sit on a grid binary16 holds exactly, so both classes keep the same values; N spans two of compact.hip's 2048-row segments
and is no multiple of 32."""
import numpy as np
import pytest
import torch

from wise_amd.index import feature_search_index as fsi
from wise_amd.index.flat_ip import FlatIPIndex
from wise_amd.index.flat_sq import FlatSQfp16IPIndex
from wise_amd.index.selector import IDSelectorBatch, SearchParameters

pytestmark = pytest.mark.gpu

N, D, NQ, K = 3000, 64, 3, 10
KINDS = {"IndexFlatIP": (lambda: FlatIPIndex(D, shadow=False), np.float32), "IndexSQfp16": (lambda: FlatSQfp16IPIndex(D), np.float16)}
kinds = pytest.mark.parametrize("kind", list(KINDS))


def grid(n, seed):
    """[n, D] float32, every value m / 64 with |m| <= 64: exact in binary16, and so is every score in fp32"""
    return (np.random.default_rng(seed).integers(-64, 65, (n, D)) / 64).astype(np.float32)


_DATA = {}


def data():
    """rows, ids (scattered, unique), queries — computed once"""
    if not _DATA:
        _DATA.update(X=grid(N, 1), ids=np.random.default_rng(2).permutation(5 * N)[:N].astype(np.int64) + 3, Q=grid(NQ, 3))
    return _DATA["X"], _DATA["ids"], _DATA["Q"]


def fresh(kind, X, ids):
    idx = KINDS[kind][0]()
    idx.add_with_ids(X, ids)
    return idx


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def host_bytes(idx, kind):
    P, I = idx.rows_host()
    assert P.dtype == KINDS[kind][1] and I.dtype == np.int64 and P.shape == (idx.ntotal, D) and I.shape == (idx.ntotal,)
    return P.tobytes(), I.tobytes()


def removed(kind):
    """(index that reserved N rows, took them in two adds and lost 400 scattered ids; bool [N] of the rows that went)"""
    X, ids, _ = data()
    a = KINDS[kind][0]()
    a.reserve(N)
    a.add_with_ids(X[:1700], ids[:1700])
    a.add_with_ids(X[1700:], ids[1700:])
    gone = np.zeros(N, bool)
    gone[np.random.default_rng(4).permutation(N)[:400]] = True
    store = a._store.reserved.data_ptr()
    assert a._store.rows.data_ptr() == store and not a._store.chunks
    assert a.remove_ids(ids[gone]) == 400 and a.ntotal == N - 400
    assert a._store.reserved.data_ptr() == store and a._store.reserved.shape[0] == N and a._store.rows.data_ptr() == store
    return a, gone


@kinds
def test_reserved_storage_survives_a_removal_and_is_filled_from_the_new_end(kind):
    X, ids, _ = data()
    a, gone = removed(kind)
    store = a._store.reserved.data_ptr()
    back = np.flatnonzero(gone)[:100]
    a.add_with_ids(X[back], ids[back])
    assert a.ntotal == N - 300 and not a._store.chunks
    assert a._store.reserved.data_ptr() == store and a._store.reserved.shape[0] == N and a._store.rows.data_ptr() == store
    order = np.concatenate([np.flatnonzero(~gone), back])
    assert host_bytes(a, kind) == host_bytes(fresh(kind, X[order], ids[order]), kind)


@kinds
def test_answers_after_a_removal_are_those_of_a_fresh_index(kind):
    X, ids, Q = data()
    a, gone = removed(kind)
    b = fresh(kind, X[~gone], ids[~gone])
    assert host_bytes(a, kind) == host_bytes(b, kind)
    params = SearchParameters(sel=IDSelectorBatch(ids[::5]))
    for p in (None, params):
        (Da, Ia), (Db, Ib) = a.search(Q, K, params=p), b.search(Q, K, params=p)
        assert Ia.shape == (NQ, K) and (Ia >= 0).all() and not np.isin(Ia, ids[gone]).any()
        assert np.array_equal(bits(Da), bits(Db)) and np.array_equal(Ia, Ib)
        assert p is None or np.isin(Ia, ids[::5]).all()
    S = Q @ X[~gone].T                                           # exact: every product and sum is a multiple of 2^-12 below 2^7
    assert np.array_equal(a.search(Q, K)[0], -np.sort(-S, axis=1)[:, :K])
    thr = float(np.sort(S[0])[-40])
    for p in (None, params):
        (la, Da, Ia), (lb, Db, Ib) = a.range_search(Q, thr, params=p), b.range_search(Q, thr, params=p)
        assert np.array_equal(la, lb) and np.array_equal(bits(Da), bits(Db)) and np.array_equal(Ia, Ib)
    assert np.array_equal(a.range_search(Q, thr)[0], np.concatenate([[0], np.cumsum((S > np.float32(thr)).sum(axis=1))]))
    ask = np.concatenate([ids[~gone][:4], ids[gone][:1], ids[~gone][-3:]])       # one id the index no longer holds
    ra, rb = a.reconstruct_batch(ask), b.reconstruct_batch(ask)
    assert np.isnan(ra[4]).all() and np.array_equal(np.delete(ra, 4, axis=0), X[~gone][[0, 1, 2, 3, -3, -2, -1]])
    assert np.array_equal(bits(ra), bits(rb))


@kinds
def test_adopt_discards_a_reservation(kind):
    """On FlatIPIndex the reservation used to survive adopt: the next add filled the old reserved tensor and replaced the
    adopted rows with it."""
    X, ids, Q = data()
    Y, Z = grid(500, 5), grid(200, 6)
    a = KINDS[kind][0]()
    a.reserve(N)
    a.add_with_ids(X[:1000], ids[:1000])
    Yd = torch.from_numpy(Y.astype(KINDS[kind][1])).cuda()
    a.adopt(Yd, None, id_base=10 ** 6)
    assert a.ntotal == 500 and a._store.reserved is None and a._store.rows.data_ptr() == Yd.data_ptr()
    z_ids = np.arange(200, dtype=np.int64) * 2 + 7
    a.add_with_ids(Z, z_ids)
    assert a.ntotal == 700
    all_ids = np.concatenate([np.arange(500, dtype=np.int64) + 10 ** 6, z_ids])
    b = fresh(kind, np.concatenate([Y, Z]), all_ids)
    assert host_bytes(a, kind) == host_bytes(b, kind)
    (Da, Ia), (Db, Ib) = a.search(Q, K), b.search(Q, K)
    assert np.array_equal(bits(Da), bits(Db)) and np.array_equal(Ia, Ib) and np.isin(Ia, all_ids).all()
    assert np.array_equal(Da, -np.sort(-(Q @ np.concatenate([Y, Z]).T), axis=1)[:, :K])


@kinds
def test_rows_host_round_trips_through_the_table(kind, tmp_path):
    X, ids, _ = data()
    entry = fsi.FLAT_TYPES[kind]
    a = fresh(kind, X, ids)
    want = host_bytes(a, kind)
    assert want == (entry.encode(X).tobytes(), ids.tobytes())
    fn, fn2 = tmp_path / "a.faiss", tmp_path / "b.faiss"
    entry.writer(fn, *a.rows_host())
    si = fsi.FeatureSearchIndex("video", "none", {"features_dir": tmp_path, "index_dir": tmp_path})
    b = si._index_from_file(fn)
    assert type(b) is type(a) and b.ntotal == N and b._store.reserved.shape[0] == N and not b._store.chunks
    assert host_bytes(b, kind) == want
    si._write_index_file(b, fn2)
    assert fn2.read_bytes() == fn.read_bytes()
    c = si._index_from_file(fn, shard=(1, 3))                    # one rank's rows of the same file
    assert host_bytes(c, kind) == (entry.encode(X[1000:2000]).tobytes(), ids[1000:2000].tobytes())

"""RowStore (wise_amd/index/flat_common.py) on the host, against plain numpy concatenation: the reserved slices, the chunks,
adopted rows and their implicit ids."""
import numpy as np
import pytest
import torch

from wise_amd.index.flat_common import RowStore

D = 16
DTYPES = [torch.float32, torch.float16]


def rows(n, seed, dtype):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)).to(dtype)


def put(store, x, ids):
    """one add: the slot, filled; returns the slot"""
    dst = store.slot(x.shape[0], ids)
    assert dst.shape == (x.shape[0], D) and dst.dtype == store.dtype
    dst.copy_(x)
    return dst


def held(store):
    store.finalize()
    assert store.rows.dtype == store.dtype and store.ids.dtype == torch.int64 and store.rows.is_contiguous()
    assert store.n == store.rows.shape[0] == store.ids.shape[0] and not store.chunks and not store.id_chunks
    return store.rows.numpy(), store.ids.numpy()


@pytest.mark.parametrize("dtype", DTYPES)
def test_reserved_slices_then_chunks(dtype):
    st = RowStore(D, dtype, "cpu")
    st.reserve(10)
    base = st.reserved.data_ptr()
    parts = [rows(4, s, dtype) for s in (1, 2, 3)]
    ids = [np.arange(4, dtype=np.int64) * 3 + 100 * s for s in (1, 2, 3)]
    a = put(st, parts[0], ids[0])
    b = put(st, parts[1], torch.from_numpy(ids[1]))              # ids as a tensor or as numpy
    assert a.data_ptr() == base and b.data_ptr() == base + 4 * D * a.element_size()
    assert st.rows.data_ptr() == base and st.n == 8 and not st.chunks and st.has_ids
    c = put(st, parts[2], ids[2])                                # 8 + 4 > 10: a chunk, and the reservation is given up
    assert st.reserved is None and len(st.chunks) == 1 and c.data_ptr() == st.chunks[0].data_ptr() and st.n == 12
    X, I = held(st)
    assert X.tobytes() == np.concatenate([p.numpy() for p in parts]).tobytes() and np.array_equal(I, np.concatenate(ids))
    with pytest.raises(ValueError, match="already holds rows"):
        st.reserve(20)


@pytest.mark.parametrize("dtype", DTYPES)
def test_adopted_rows_get_their_implicit_ids_once_rows_follow(dtype):
    st = RowStore(D, dtype, "cpu")
    A, B = rows(9, 4, dtype), rows(5, 5, dtype)
    st.adopt(A, None, id_base=7)
    assert st.rows.data_ptr() == A.data_ptr() and st.ids is None and st.id_base == 7 and st.n == 9 and not st.has_ids
    assert np.array_equal(st.explicit_ids().numpy(), np.arange(7, 16)) and st.ids is None
    new = np.array([1000, 3, 5, 999, 4], dtype=np.int64)
    put(st, B, new)
    assert st.n == 14 and st.has_ids
    X, I = held(st)
    assert X.tobytes() == np.concatenate([A.numpy(), B.numpy()]).tobytes()
    assert np.array_equal(I, np.concatenate([np.arange(7, 7 + 9), new]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_adopt_discards_a_reservation(dtype):
    st = RowStore(D, dtype, "cpu")
    st.reserve(20)
    first = rows(6, 6, dtype)
    put(st, first, np.arange(6))
    old, old_ids = st.reserved, st.reserved_ids
    before, before_ids = old.clone(), old_ids.clone()
    A, B = rows(7, 7, dtype), rows(3, 8, dtype)
    A_ids = torch.arange(7, dtype=torch.int64) + 50
    st.adopt(A, A_ids)
    assert st.reserved is None and st.reserved_ids is None and st.n == 7 and st.rows.data_ptr() == A.data_ptr()
    put(st, B, np.array([90, 91, 92]))                           # 6 + 3 rows would have fitted the old reservation
    X, I = held(st)
    assert X.tobytes() == np.concatenate([A.numpy(), B.numpy()]).tobytes()
    assert np.array_equal(I, np.concatenate([A_ids.numpy(), [90, 91, 92]]))
    assert old[:6].numpy().tobytes() == first.numpy().tobytes()  # the old reserved tensors are not written
    assert old.view(torch.uint8).equal(before.view(torch.uint8)) and old_ids.equal(before_ids)


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_store(dtype):
    st = RowStore(D, dtype, "cpu")
    assert st.n == 0 and not st.has_ids
    X, I = held(st)
    assert X.shape == (0, D) and I.shape == (0,) and st.explicit_ids().shape == (0,)
    st.reserve(4)                                                # an empty store still takes a reservation, and rows
    x = rows(3, 9, dtype)
    put(st, x, np.array([5, 6, 7]))
    X, I = held(st)
    assert X.tobytes() == x.numpy().tobytes() and np.array_equal(I, [5, 6, 7]) and st.rows.data_ptr() == st.reserved.data_ptr()


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals(dtype):
    st = RowStore(D, dtype, "cpu")
    for bad in (np.arange(3), np.arange(5), np.zeros((4, 1), np.int64), torch.arange(3)):
        with pytest.raises(ValueError, match="add_with_ids: ids must have one entry per row"):
            st.slot(4, bad)
    with pytest.raises(ValueError, match="add_halves_with_ids: ids must have one entry per row"):
        st.slot(4, np.arange(3), "add_halves_with_ids")
    assert st.n == 0 and not st.chunks
    other = torch.float16 if dtype == torch.float32 else torch.float32
    for bad in (rows(4, 1, other), torch.zeros(4, D + 1, dtype=dtype), torch.zeros(4 * D, dtype=dtype),
                torch.zeros(4, 2 * D, dtype=dtype)[:, ::2], torch.zeros(D, 4, dtype=dtype).t()):
        with pytest.raises(ValueError, match="adopt: rows must be contiguous"):
            st.adopt(bad)
    for bad_ids in (torch.arange(3), torch.arange(4, dtype=torch.int32)):
        with pytest.raises(ValueError, match="adopt: ids must be int64"):
            st.adopt(torch.zeros(4, D, dtype=dtype), bad_ids)
    assert st.n == 0 and st.rows is None
    named = RowStore(D, dtype, "cpu", what="X must be contiguous float32 [N,d]")
    with pytest.raises(ValueError, match=r"adopt: X must be contiguous float32 \[N,d\]"):
        named.adopt(torch.zeros(4, D + 1, dtype=dtype))

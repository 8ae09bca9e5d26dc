"""-m gpu: the group selector, faiss's IDSelectorBitmap and the And / Or / XOr / Not trees (csrc/sel_tree.hip,
wise_amd/index/selector.py), bit for bit.

(1) wise_sel_bitmap_groups, wise_sel_bitmap_idbits and wise_sel_combine alone: every bitmap word against tests/sel_tree_ref.py, at
    the sizes around a word, a wave and a block; (2) every index type end to end against an oracle the new code does not touch: the
    same index's search under IDSelectorBatch of the ids the restatement selects — the path that existed before — must give the same
    (D, I) bits as the search under the tree, and so for range_search and search_grouped; (3) remove_ids(IDSelectorGroups(keys))
    against remove_ids(expanded ids); (4) the refusals on real indexes; (5) FeatureSearchIndex.remove_groups on index files."""
import numpy as np
import pytest
import torch

import sel_tree_ref as ref
from wise_amd import _lib
from wise_amd.index.selector import (IDSelectorAll, IDSelectorAnd, IDSelectorArray, IDSelectorBatch, IDSelectorBitmap, IDSelectorGroups,
                                     IDSelectorNot, IDSelectorOr, IDSelectorRange, IDSelectorXOr, SearchParameters, SearchParametersIVF)

pytestmark = pytest.mark.gpu
WISE_E_INVALID = -1
SIZES = [0, 1, 31, 32, 33, 63, 64, 65, 4133]
JUNK = 0x5A5A5A5A                                                                       # what an output holds before a call


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _junk(N, pad=0):
    return torch.full(((N + 31) // 32 + pad,), JUNK, dtype=torch.int32, device="cuda")


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _bits(a):
    a = np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))


# ---- (1) the three entry points alone
def _layouts(rng, N, G):
    """[N] int64 group of every row (every group has a row), as contiguous runs and the same permuted over the rows; where the
    sizes allow it group 0 is a single row (row 0) and group 1 straddles the 64-row boundary (rows 1 .. 66)"""
    if N == 0:
        return [np.empty(0, np.int64)]
    length, extra, others = np.ones(G, dtype=np.int64), N - G, np.arange(G)
    if G >= 3 and extra >= 65:
        length[1] += 65
        extra, others = extra - 65, np.arange(2, G)
    length[others] += rng.multinomial(extra, np.full(others.size, 1.0 / others.size))
    runs = np.repeat(np.arange(G, dtype=np.int64), length)
    assert runs.size == N and (G < 3 or N - G < 65 or ((runs == 0).sum() == 1 and runs[63] == runs[64] == 1))
    return [runs, rng.permutation(runs)]


def _groups(lib, gid, group_keys, sel_keys, invert, N):
    G = group_keys.size
    d_gid, d_keys, d_sel = _dev(gid.astype(np.int32)), _dev(group_keys), _dev(sel_keys)
    out = _junk(N)
    need = lib.wise_sel_groups_workspace_bytes(G)
    assert need > 0 and need % 256 == 0
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")                     # stale marks from another call
    _lib.check(lib.wise_sel_bitmap_groups(d_gid.data_ptr(), N, d_keys.data_ptr(), G, d_sel.data_ptr(), sel_keys.size, invert, out.data_ptr(),
                                          ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "wise_sel_bitmap_groups")
    return _words(out)


@pytest.mark.parametrize("N", SIZES)
def test_groups_bitmap_alone(N):
    lib = _lib.lib()
    rng = np.random.default_rng(100 + N)
    for G in sorted({g for g in (1, 97, N) if g <= N} | ({0} if N == 0 else set())):
        group_keys = np.sort(rng.choice(np.arange(0, 10 * G + 10), G, replace=False)).astype(np.int64) * 7 + 3    # ascending, with gaps
        absent = np.array([-5, 1, 10 ** 12], dtype=np.int64)                            # keys are 3 mod 7: no group carries these
        selections = [np.empty(0, np.int64), absent] + ([] if G == 0 else [group_keys[G // 2:G // 2 + 1], group_keys,
                                                                          np.sort(np.concatenate([group_keys[::3], absent]))])
        for gid in _layouts(rng, N, G):
            for sel_keys in selections:                                                 # n_sel 0, 1, G, and keys no group carries
                for invert in (0, 1):
                    want = ref.words(ref.groups_mask(gid, group_keys, sel_keys) != bool(invert))
                    got = _groups(lib, gid, group_keys, sel_keys, invert, N)
                    assert np.array_equal(got, want), (N, G, sel_keys.size, invert)
    if N:                                                                               # gid outside [0, G) is no group: never selected
        gid = rng.integers(-2, 9, N)
        group_keys = np.arange(5, dtype=np.int64)
        for invert in (0, 1):
            want = ref.words(ref.groups_mask(gid, group_keys, group_keys) != bool(invert))
            assert np.array_equal(_groups(lib, gid, group_keys, group_keys, invert, N), want)
        # G = 0 with rows: no row has a group
        none = np.empty(0, np.int64)
        assert np.array_equal(_groups(lib, gid, none, none, 0, N), ref.words(np.zeros(N, bool)))
        assert np.array_equal(_groups(lib, gid, none, none, 1, N), ref.words(np.ones(N, bool)))


def test_groups_bitmap_same_bits_on_every_run():
    lib = _lib.lib()
    rng = np.random.default_rng(1)
    N, G = 4133, 97
    gid, group_keys = rng.integers(0, G, N), np.arange(G, dtype=np.int64) * 2
    first = _groups(lib, gid, group_keys, group_keys[::2], 0, N)
    for _ in range(3):
        assert np.array_equal(_groups(lib, gid, group_keys, group_keys[::2], 0, N), first)


@pytest.mark.parametrize("N", SIZES)
def test_idbits_alone(N):
    lib = _lib.lib()
    rng = np.random.default_rng(200 + N)
    st = _lib.stream_ptr()
    explicit = rng.permutation(N).astype(np.int64) * 3 - 40                             # negative ids, and ids beyond any bitmap here
    for ids, id_base in ((explicit, 0), (None, 0), (None, 1000), (None, -17)):
        rid = ref.row_ids(ids, id_base, N)
        d_ids = None if ids is None else _dev(ids)
        for n_bytes in (0, 1, 37, (3 * N + 7) // 8 + 200):                              # none, ids 0 .. 7, a part, every id and more
            bits = rng.integers(0, 256, n_bytes).astype(np.uint8)
            d_bits = _dev(bits) if n_bytes else None
            for invert in (0, 1):
                out = _junk(N)
                _lib.check(lib.wise_sel_bitmap_idbits(_lib.ptr(d_ids), id_base, N, _lib.ptr(d_bits), n_bytes, invert, out.data_ptr(), st),
                           "wise_sel_bitmap_idbits")
                want = ref.words(ref.idbits_mask(rid, bits) != bool(invert))
                assert np.array_equal(_words(out), want), (N, id_base, n_bytes, invert)


@pytest.mark.parametrize("N", SIZES + [40_001])                                          # 40,001: more than one block of the combine pass
def test_combine_alone(N):
    lib = _lib.lib()
    rng = np.random.default_rng(300 + N)
    st = _lib.stream_ptr()
    nw = (N + 31) // 32
    a = rng.integers(0, 2 ** 32, nw, dtype=np.uint64).astype(np.uint32)                 # random words: the inputs' tails are dirty
    b = rng.integers(0, 2 ** 32, nw, dtype=np.uint64).astype(np.uint32)
    for op in range(5):
        want = ref.combine(a, b, N, op)
        if N & 31 and nw:
            assert want[-1] >> (N & 31) == 0                                            # the tail is zero for every op
        for alias in ("new", "a", "b", "unaligned"):
            pad = 1 if alias == "unaligned" else 0                                      # a view one word in: 4-byte aligned only
            d_a, d_b = _junk(N, pad)[pad:], _junk(N, pad)[pad:]
            d_a.copy_(_dev(a.view(np.int32)))
            d_b.copy_(_dev(b.view(np.int32)))
            out = {"new": _junk(N), "a": d_a, "b": d_b, "unaligned": _junk(N, 1)[1:]}[alias]
            _lib.check(lib.wise_sel_combine(d_a.data_ptr(), 0 if op == 4 and alias != "b" else d_b.data_ptr(), N, op, out.data_ptr(), st),
                       "wise_sel_combine")
            assert np.array_equal(_words(out), want), (N, op, alias)
            if alias == "new":                                                          # the inputs are left alone
                assert np.array_equal(_words(d_a), a) and np.array_equal(_words(d_b), b)
    if N in (33, 4133):                                                                 # the tail after NOT and XOR, on clean inputs too
        m = rng.random(N) < 0.5
        d_m = _dev(ref.words(m).view(np.int32))
        out = _junk(N)
        _lib.check(lib.wise_sel_combine(d_m.data_ptr(), 0, N, 4, out.data_ptr(), st), "not")
        assert np.array_equal(_words(out), ref.words(~m)) and _words(out)[-1] >> (N & 31) == 0
        ones = _dev(ref.words(np.ones(N, bool)).view(np.int32))
        full = torch.full_like(ones, -1)                                                # all ones with a dirty tail
        _lib.check(lib.wise_sel_combine(d_m.data_ptr(), full.data_ptr(), N, 2, out.data_ptr(), st), "xor")
        assert np.array_equal(_words(out), ref.words(~m))


def test_bad_arguments_write_nothing():
    lib = _lib.lib()
    st = _lib.stream_ptr()
    N, G = 100, 5
    gid, keys = _dev(np.arange(N, dtype=np.int32) % G), _dev(np.arange(G, dtype=np.int64))
    out, ws = _junk(N), torch.zeros(256, dtype=torch.uint8, device="cuda")
    good = [gid.data_ptr(), N, keys.data_ptr(), G, keys.data_ptr(), G, 0, out.data_ptr(), ws.data_ptr(), 256, st]
    for at, val in ((1, -1), (1, 0xFFFFFFFF), (3, -1), (5, -1), (0, 0), (2, 0), (4, 0), (8, 0), (9, 255)):
        args = list(good)
        args[at] = val
        assert lib.wise_sel_bitmap_groups(*args) == WISE_E_INVALID and lib.wise_last_error(), (at, val)
    ids = _dev(np.arange(N, dtype=np.int64))
    assert lib.wise_sel_bitmap_idbits(ids.data_ptr(), 0, N, 0, 4, 0, out.data_ptr(), st) == WISE_E_INVALID
    assert lib.wise_sel_bitmap_idbits(ids.data_ptr(), 0, N, ws.data_ptr(), -1, 0, out.data_ptr(), st) == WISE_E_INVALID
    src = _dev(np.zeros(4, dtype=np.int32))
    for args in ((src.data_ptr(), src.data_ptr(), N, 5, out.data_ptr(), st), (src.data_ptr(), 0, N, 1, out.data_ptr(), st),
                 (0, src.data_ptr(), N, 0, out.data_ptr(), st), (src.data_ptr(), src.data_ptr(), -1, 0, out.data_ptr(), st)):
        assert lib.wise_sel_combine(*args) == WISE_E_INVALID
    torch.cuda.synchronize()
    assert bool((out == JUNK).all()) and bool((ws == 0).all())
    _lib.check(lib.wise_sel_bitmap_groups(*good), "wise_sel_bitmap_groups")             # and the good call works
    assert np.array_equal(_words(out), ref.words(np.ones(N, bool)))


# ---- (2) every index type end to end: the search under IDSelectorBatch of the expanded ids is the oracle
N_ROWS, DIM, NLIST = 4133, 64, 16
FLAT = ["IndexFlatIP", "IndexSQfp16", "IndexSQ8bit", "IndexFlatL2", "IndexSQfp16L2"]
IVF = ["IndexIVFFlat", "IndexIVFSQ8", "IndexIVFSQfp16", "IndexIVFFlatL2"]
PQ = ["IndexIVFPQ16", "IndexPQ16"]


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(42)
    X = rng.standard_normal((N_ROWS, DIM)).astype(np.float32)
    X[N_ROWS // 2] = X[5]                                                               # equal scores: the tie rule decides
    ids = rng.permutation(N_ROWS).astype(np.int64) * 3 + 7                              # 7 .. 12403, not the positions
    runs = np.sort(np.concatenate([np.arange(60), rng.integers(0, 60, N_ROWS - 60)]))   # 60 videos of uneven length, in add order
    keys_of_rows = runs.astype(np.int64) * 5 + 2
    Q = (X[rng.integers(0, N_ROWS, 5)] + 0.25 * rng.standard_normal((5, DIM))).astype(np.float32)
    Q[0] = X[5]
    group_keys, gid = np.unique(keys_of_rows, return_inverse=True)
    return dict(X=X, ids=ids, keys=keys_of_rows, Q=Q, group_keys=group_keys, gid=gid.reshape(-1), bits=rng.integers(0, 256, 800).astype(np.uint8))


def _make(name, X, ids):
    from wise_amd.index.flat_ip import FlatIPIndex
    from wise_amd.index.flat_l2 import FlatL2Index
    from wise_amd.index.flat_pq import FlatPQIPIndex
    from wise_amd.index.flat_sq import FlatSQ8IPIndex, FlatSQfp16IPIndex, FlatSQfp16L2Index
    from wise_amd.index.ivf_flat import IVFFlatIPIndex, IVFFlatL2Index
    from wise_amd.index.ivf_pq import IVFPQIPIndex
    from wise_amd.index.ivf_sq import IVFSQfp16IPIndex, IVFSQIPIndex
    d = X.shape[1]
    flat = {"IndexFlatIP": FlatIPIndex, "IndexSQfp16": FlatSQfp16IPIndex, "IndexSQ8bit": FlatSQ8IPIndex, "IndexFlatL2": FlatL2Index,
            "IndexSQfp16L2": FlatSQfp16L2Index}
    ivf = {"IndexIVFFlat": IVFFlatIPIndex, "IndexIVFSQ8": IVFSQIPIndex, "IndexIVFSQfp16": IVFSQfp16IPIndex, "IndexIVFFlatL2": IVFFlatL2Index}
    if name in flat:
        ix = flat[name](d)
        if name == "IndexSQ8bit":
            ix.train(X)
    elif name in ivf:
        ix = ivf[name](d, NLIST)
        ix.train(X)
    elif name == "IndexIVFPQ16":
        ix = IVFPQIPIndex(d, NLIST, 16)
        ix.train(X)
    else:
        ix = FlatPQIPIndex(d, 16)
        ix.train(X)
    ix.add_with_ids(X, ids)
    return ix


def _trees(data, with_groups):
    """name -> a fresh tree; the ones with a group selector only where the type takes groups"""
    ids, gk = data["ids"], data["group_keys"]
    lo, hi = int(np.sort(ids)[N_ROWS // 5]), int(np.sort(ids)[N_ROWS // 2])
    some = np.concatenate([gk[::3], gk[:2], [1, -9]])                                   # duplicates, and keys no group carries
    trees = {
        "batch or bitmap": IDSelectorOr(IDSelectorBatch(ids[::7]), IDSelectorBitmap(data["bits"])),       # ids 6400 and up: beyond the bitmap
        "not of an and": IDSelectorNot(IDSelectorAnd(IDSelectorArray(ids[::2]), IDSelectorRange(lo, hi))),
        "all": IDSelectorAll(),
    }
    if with_groups:
        trees.update({
            "groups": IDSelectorGroups(some),
            "groups and not range": IDSelectorAnd(IDSelectorGroups(some), IDSelectorNot(IDSelectorRange(lo, hi))),
            "xor of two group sets": IDSelectorXOr(IDSelectorGroups(gk[::2]), IDSelectorGroups(gk[1::3])),
            "not of an and with groups": IDSelectorNot(IDSelectorAnd(IDSelectorGroups(gk[5:40]), IDSelectorBitmap(data["bits"]))),
            "one video": IDSelectorGroups([int(gk[7])]),
            "no video": IDSelectorGroups([1, -9]),
        })
    return trees


def _expanded(data, tree):
    """the ids the restatement selects (selection is a function of a row's id and group, so the add order serves every index)"""
    m = ref.mask(tree, data["ids"], 0, N_ROWS, data["gid"], data["group_keys"])
    return data["ids"][m], m


def _check_type(name, data):
    ivf, groups = name in IVF or name == "IndexIVFPQ16", name not in PQ
    ix = _make(name, data["X"], data["ids"])
    if groups:
        ix.set_groups(data["ids"], data["keys"])
    P = (lambda sel: SearchParametersIVF(sel=sel, nprobe=4)) if ivf else (lambda sel: SearchParameters(sel=sel))
    counts = {}
    for tname, tree in _trees(data, groups).items():
        chosen, m = _expanded(data, tree)
        counts[tname] = int(m.sum())
        oracle = IDSelectorBatch(chosen)
        for nq in (1, 5):
            x = data["Q"][:nq]
            for k in (1, 10, 100):
                assert _same(ix.search(x, k, params=P(tree)), ix.search(x, k, params=P(oracle))), (name, tname, nq, k)
            if name in PQ:
                continue
            D10 = ix.search(x, 10, params=P(None) if ivf else None)[0]
            thresh = float(D10[0, 9])                                                   # a handful of hits a query, fewer under the filter
            assert _same(ix.range_search(x, thresh, params=P(tree)), ix.range_search(x, thresh, params=P(oracle))), (name, tname, nq)
            for k in (1, 10, 100):
                assert _same(ix.search_grouped(x, k, params=P(tree)), ix.search_grouped(x, k, params=P(oracle))), (name, tname, nq, k)
        if not ivf and name not in PQ:                                                  # every selected row, and only those, can be returned
            if m.sum() <= 2000:
                got = ix.search(data["Q"][:1], 2000, params=P(tree))[1][0]
                assert sorted(got[got >= 0].tolist()) == sorted(chosen.tolist()), (name, tname)
    assert counts["all"] == N_ROWS and 0 < counts["batch or bitmap"] < N_ROWS
    if groups:
        assert counts["no video"] == 0 and 0 < counts["one video"] < 400 and 0 < counts["groups"] < N_ROWS
    return ix


@pytest.mark.parametrize("name", FLAT + IVF)
def test_trees_against_the_batch_selector(name, data):
    ix = _check_type(name, data)
    # rows changed after set_groups: the RuntimeError of search_grouped, from the selector too
    ix.add_with_ids(data["X"][:3], np.array([50_000, 50_001, 50_002]))
    P = SearchParametersIVF if name in IVF else SearchParameters
    for tree in (IDSelectorGroups([2]), IDSelectorOr(IDSelectorAll(), IDSelectorNot(IDSelectorGroups([2])))):
        with pytest.raises(RuntimeError, match="set_groups"):
            ix.search(data["Q"][:1], 5, params=P(sel=tree))
    assert ix.search(data["Q"][:1], 5, params=P(sel=IDSelectorAll()))[1].shape == (1, 5)  # a tree without groups still resolves


@pytest.mark.parametrize("name", PQ)
def test_pq_types_take_trees_without_groups_and_refuse_groups(name, data):
    ix = _check_type(name, data)
    P = SearchParametersIVF if name == "IndexIVFPQ16" else SearchParameters
    for tree in (IDSelectorGroups([2]), IDSelectorAnd(IDSelectorAll(), IDSelectorGroups([2]))):
        with pytest.raises(NotImplementedError, match="product-quantized"):
            ix.search(data["Q"][:1], 5, params=P(sel=tree))
        with pytest.raises(NotImplementedError, match="product-quantized"):
            ix.remove_ids(tree)


# ---- (3) remove_ids(IDSelectorGroups(keys)) is remove_ids(expanded ids)
@pytest.mark.parametrize("name", FLAT + IVF)
def test_remove_ids_of_groups(name, data):
    ivf = name in IVF
    a, b = _make(name, data["X"], data["ids"]), _make(name, data["X"], data["ids"])
    a.set_groups(data["ids"], data["keys"])
    keys = np.concatenate([data["group_keys"][3:30:4], [data["group_keys"][3], 1]])      # a duplicate and a key no group carries
    sel = IDSelectorGroups(keys)
    chosen, m = _expanded(data, sel)
    assert 0 < m.sum() < N_ROWS
    assert a.remove_ids(sel) == b.remove_ids(chosen) == int(m.sum())
    assert a.ntotal == b.ntotal == N_ROWS - int(m.sum())
    P = (lambda: SearchParametersIVF(nprobe=NLIST)) if ivf else (lambda: None)
    for nq in (1, 5):
        for k in (1, 10, 100):
            got, want = a.search(data["Q"][:nq], k, params=P()), b.search(data["Q"][:nq], k, params=P())
            assert _same(got, want) and not np.isin(got[1], chosen).any(), (name, nq, k)
    gone = np.isin(data["ids"], chosen)
    assert np.array_equal(a.reconstruct_batch(data["ids"][gone][:4]).view(np.int32), b.reconstruct_batch(data["ids"][gone][:4]).view(np.int32))
    with pytest.raises(RuntimeError, match="set_groups"):                               # the removal changed the rows: the tables went
        a.remove_ids(sel)
    a.set_groups(data["ids"], data["keys"])                                             # extra ids (the removed ones) are ignored
    assert a.remove_ids(sel) == 0 and a.ntotal == b.ntotal


# ---- (5) FeatureSearchIndex.remove_groups on index files
@pytest.mark.parametrize("name", ["IndexFlatIP", "IndexIVFSQ8"])
def test_remove_groups_rewrites_the_file(name, data, tmp_path, capsys):
    from wise_amd.index.feature_search_index import FeatureSearchIndex
    si = FeatureSearchIndex("video", "extractor", {"features_dir": str(tmp_path), "index_dir": str(tmp_path)})
    fn = si.get_index_filename(name)
    FeatureSearchIndex._write_index_file(_make(name, data["X"], data["ids"]), fn)
    si.index = si._index_from_file(fn)
    with pytest.raises(RuntimeError, match="set_groups"):
        si.remove_groups(name, [2])
    si.set_groups(data["ids"], data["keys"])
    keys = data["group_keys"][[4, 9, 9, 31]]
    chosen, m = _expanded(data, IDSelectorGroups(keys))
    assert si.remove_groups(name, keys) == int(m.sum()) > 0
    assert not list(tmp_path.glob("*.tmp-*"))
    left = si._index_from_file(fn)
    kept = np.sort(left._selector_rows()[0].cpu().numpy())
    assert np.array_equal(kept, np.sort(data["ids"][~m]))
    want = _make(name, data["X"], data["ids"])                                          # the file's index is the one left by remove_ids(ids)
    want.remove_ids(chosen)
    assert _same(left.search(data["Q"], 10), want.search(data["Q"], 10))
    before = fn.stat().st_mtime_ns
    si.index = left
    si.set_groups(data["ids"], data["keys"])
    assert si.remove_groups(name, [1, -9]) == 0 and fn.stat().st_mtime_ns == before       # nothing to remove: the file is left alone

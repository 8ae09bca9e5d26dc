"""No GPU: the host side of the group selector and of selector trees (wise_amd/index/selector.py, csrc/sel_tree.hip) — constructor
validation, the recursion over a tree against tests/sel_tree_ref.py with the four launches stood in for by numpy, the cache and its
key, the refusals, FeatureSearchIndex's `within_groups`, the declarations of the new entry points under ABI 5, and every
WISE_E_INVALID path of theirs, which must answer before any device is looked at."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import sel_tree_ref as ref
from wise_amd.index import selector as S
from wise_amd.index.selector import (IDSelector, IDSelectorAll, IDSelectorAnd, IDSelectorArray, IDSelectorBatch, IDSelectorBitmap,
                                     IDSelectorGroups, IDSelectorNot, IDSelectorOr, IDSelectorRange, IDSelectorXOr, ResolvedSelector,
                                     SearchParameters, as_selector, resolve_for, within_selector)

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = {"wise_sel_groups_workspace_bytes": 1, "wise_sel_bitmap_groups": 11, "wise_sel_bitmap_idbits": 8, "wise_sel_combine": 6}


# ------------------------------------------------------------------------------------------------------------------ constructors
def test_constructors_validate():
    g = IDSelectorGroups(np.array([[7, 3], [7, 9]]))
    assert g.keys.dtype == np.int64 and g.keys.tolist() == [7, 3, 7, 9]                # flattened, duplicates kept as given
    assert IDSelectorGroups([]).keys.shape == (0,) and IDSelectorGroups(torch.tensor([4, 2])).keys.tolist() == [4, 2]
    assert IDSelectorArray([5, 5, 1]).ids.tolist() == [5, 5, 1] and isinstance(IDSelectorArray([1]), IDSelectorBatch)
    b = IDSelectorBitmap(np.array([1, 255], dtype=np.uint8))
    assert b.bits.dtype == np.uint8 and b.bits.tolist() == [1, 255] and IDSelectorBitmap(np.empty(0, np.uint8)).bits.size == 0
    for bad in (lambda: IDSelectorGroups([1.5, 2.0]), lambda: IDSelectorGroups(["a"]), lambda: IDSelectorArray([0.5]),
                lambda: IDSelectorBitmap([1, 2, 3]), lambda: IDSelectorBitmap(np.array([0.5])), lambda: IDSelectorBitmap(np.array([1, 2], np.int8))):
        with pytest.raises(ValueError):
            bad()
    r = IDSelectorRange(0, 5)
    for cls in (IDSelectorAnd, IDSelectorOr, IDSelectorXOr):
        node = cls(g, r)
        assert node.lhs is g and node.rhs is r and isinstance(node, IDSelector)
        for lhs, rhs in (([1, 2], r), (r, None), (r, ResolvedSelector(torch.zeros(1, dtype=torch.int32), 5)), (np.arange(3), np.arange(3))):
            with pytest.raises(ValueError, match="expected two IDSelectors"):
                cls(lhs, rhs)                                                          # an id list is not a selector here
    n = IDSelectorNot(IDSelectorAnd(g, IDSelectorNot(r)))                              # Not takes a compound selector
    assert isinstance(n.sel, IDSelectorAnd) and IDSelectorNot(IDSelectorAll()).sel._spec("cpu")[4] is True
    with pytest.raises(ValueError):
        IDSelectorNot(np.arange(3))
    assert SearchParameters(sel=n).sel is n and as_selector(n) is n
    # which trees belong to one state of the group tables
    assert n._uses_groups() and IDSelectorOr(r, IDSelectorXOr(b, IDSelectorNot(g)))._uses_groups() and g._uses_groups()
    assert not IDSelectorOr(r, IDSelectorNot(b))._uses_groups() and not IDSelectorAll()._uses_groups() and not r._uses_groups()
    # the existing classes' _spec stays what it was
    assert IDSelectorNot(r)._spec("cpu") == (S.MODE_RANGE, None, 0, 5, True) and IDSelectorNot(IDSelectorNot(r))._spec("cpu")[4] is False
    mode, ids, _, _, inv = IDSelectorArray([3, 1, 3])._spec("cpu")
    assert mode == S.MODE_BATCH and ids.tolist() == [1, 3] and inv is False


# ------------------------------------------------------------------------------------------- the recursion, launches stood in for
class _Index:
    """an index as far as selector resolution looks at it, with group tables"""
    device = "cpu"

    def __init__(self, ids, id_base, n, gid, group_keys):
        self.ids = None if ids is None else torch.from_numpy(np.asarray(ids, dtype=np.int64))
        self.id_base, self.n, self.version, self._mutations, self.asked = id_base, n, 0, 0, 0
        self.tables = dict(n=n, gid=torch.from_numpy(np.asarray(gid, dtype=np.int32)), keys=torch.from_numpy(np.asarray(group_keys, dtype=np.int64)))

    def _selector_rows(self):
        return self.ids, self.id_base, self.n

    def _rows_version(self):
        return self.version

    def _need_groups(self):
        self.asked += 1
        if self.tables is None:
            raise RuntimeError("call set_groups(ids, keys) first")
        return self.tables


def _t(w):
    return torch.from_numpy(np.ascontiguousarray(w).view(np.int32).copy())


def _w(t):
    return t.numpy().view(np.uint32)


@pytest.fixture
def launches(monkeypatch):
    """the four places selector.py reaches the library, restated in numpy over host tensors; returns the log of launches"""
    log = []

    def leaf(ids, id_base, n, spec, device):
        mode, sorted_ids, imin, imax, invert = spec
        rid = ref.row_ids(None if ids is None else ids.numpy(), id_base, n)
        if mode == S.MODE_RANGE:
            m = (rid >= imin) & (rid < imax)
        else:
            have = np.empty(0, np.int64) if sorted_ids is None else sorted_ids.numpy()
            assert np.array_equal(have, np.unique(have))                               # sorted, without duplicates
            m = np.isin(rid, have)
        log.append(("bitmap", bool(invert)))
        return _t(ref.words(m != bool(invert)))

    def groups(tables, n, sel_keys, invert, device):
        keys = sel_keys.numpy()
        assert np.array_equal(keys, np.unique(keys)) and keys.dtype == np.int64
        log.append(("groups", bool(invert)))
        return _t(ref.words(ref.groups_mask(tables["gid"].numpy(), tables["keys"].numpy(), keys) != bool(invert)))

    def idbits(ids, id_base, n, bits, invert, device):
        rid = ref.row_ids(None if ids is None else ids.numpy(), id_base, n)
        log.append(("idbits", bool(invert)))
        return _t(ref.words(ref.idbits_mask(rid, bits.numpy()) != bool(invert)))

    def combine(a, b, n, op, out=None):
        log.append(("combine", op))
        r = _t(ref.combine(_w(a), None if b is None else _w(b), n, op))
        if out is None:
            return r
        out.copy_(r)
        return out

    monkeypatch.setattr(S, "_leaf_bitmap", leaf)
    monkeypatch.setattr(S, "_groups_bitmap", groups)
    monkeypatch.setattr(S, "_idbits_bitmap", idbits)
    monkeypatch.setattr(S, "_combine", combine)
    return log


def _case(n, G, explicit, seed=0):
    rng = np.random.default_rng(seed + n)
    ids = (rng.permutation(n).astype(np.int64) * 2 + 3) if explicit else None
    gid = rng.integers(0, G, n) if n else np.empty(0, np.int64)
    group_keys = np.arange(G, dtype=np.int64) * 5 + 1
    return _Index(ids, 40, n, gid, group_keys), gid, group_keys


def _trees(ix, group_keys, rng):
    n = ix.n
    rid = ref.row_ids(None if ix.ids is None else ix.ids.numpy(), ix.id_base, n)
    lo, hi = (int(np.sort(rid)[n // 4]), int(np.sort(rid)[n // 2])) if n else (0, 0)
    some = group_keys[::3]
    bits = rng.integers(0, 256, 12).astype(np.uint8)                                   # ids 0 .. 95; the rest are beyond the bitmap
    groups = lambda: IDSelectorGroups(np.concatenate([some, some[:2], [2, -4]]))       # duplicates, keys no group carries
    rng_sel, batch = (lambda: IDSelectorRange(lo, hi)), (lambda: IDSelectorBatch(rid[::5]))
    return {                                                                           # name: (tree, launches as the stand-ins count them)
        "groups": (groups(), 1),
        "not groups": (IDSelectorNot(groups()), 1),
        "groups and not range": (IDSelectorAnd(groups(), IDSelectorNot(rng_sel())), 3),
        "batch or bitmap": (IDSelectorOr(batch(), IDSelectorBitmap(bits)), 3),
        "xor of two group sets": (IDSelectorXOr(IDSelectorGroups(group_keys[::2]), IDSelectorGroups(group_keys[1::3])), 3),
        "not of an and": (IDSelectorNot(IDSelectorAnd(IDSelectorArray(rid[::2]), rng_sel())), 4),
        "all": (IDSelectorAll(), 1),
        "not not bitmap": (IDSelectorNot(IDSelectorNot(IDSelectorBitmap(bits))), 1),
        "deep": (IDSelectorOr(IDSelectorAnd(IDSelectorNot(groups()), IDSelectorAll()),
                              IDSelectorXOr(IDSelectorNot(IDSelectorOr(batch(), rng_sel())), groups())), 10),
    }


@pytest.mark.parametrize("explicit", [True, False])
@pytest.mark.parametrize("n,G", [(0, 1), (1, 1), (33, 4), (64, 64), (4133, 97)])
def test_the_recursion_against_the_restatement(launches, n, G, explicit):
    ix, gid, group_keys = _case(n, G, explicit)
    for name, (tree, count) in _trees(ix, group_keys, np.random.default_rng(n)).items():
        launches.clear()
        res = tree.resolve(ix)
        want = ref.words(ref.mask(tree, None if ix.ids is None else ix.ids.numpy(), ix.id_base, n, gid, group_keys))
        assert isinstance(res, ResolvedSelector) and res.n == n and res.bitmap.dtype == torch.int32, name
        assert np.array_equal(_w(res.bitmap), want), name
        assert len(launches) == count, (name, launches)                                # one launch a node; a Not over a leaf is none
        assert tree.resolve(ix) is res and len(launches) == count, name                # cached: nothing runs again
        assert resolve_for(ix, tree) is res


def test_not_folds_into_the_leaf_and_and_not_is_one_pass(launches):
    ix, gid, group_keys = _case(100, 7, True)
    IDSelectorNot(IDSelectorGroups([1])).resolve(ix)
    IDSelectorNot(IDSelectorNot(IDSelectorBatch([3]))).resolve(ix)
    IDSelectorNot(IDSelectorBitmap(np.ones(4, np.uint8))).resolve(ix)
    assert launches == [("groups", True), ("bitmap", False), ("idbits", True)]
    launches.clear()
    IDSelectorAnd(IDSelectorRange(0, 50), IDSelectorNot(IDSelectorGroups([6]))).resolve(ix)
    assert launches == [("bitmap", False), ("groups", False), ("combine", S.OP_ANDNOT)]
    launches.clear()
    IDSelectorNot(IDSelectorOr(IDSelectorRange(0, 50), IDSelectorAll())).resolve(ix)
    assert launches == [("bitmap", False), ("bitmap", True), ("combine", S.OP_OR), ("combine", S.OP_NOT)]
    # a subtree shared by two filters is resolved once
    launches.clear()
    shared = IDSelectorGroups([1, 6])
    a, b = IDSelectorAnd(shared, IDSelectorRange(0, 50)), IDSelectorOr(IDSelectorRange(10, 20), shared)
    a.resolve(ix), b.resolve(ix)
    assert [what for what, _ in launches].count("groups") == 1 and a.resolve(ix).bitmap is not shared.resolve(ix).bitmap


def test_the_cache_keys_on_the_rows_version_for_group_selectors(launches):
    ix, gid, group_keys = _case(200, 9, True)
    plain = IDSelectorOr(IDSelectorRange(0, 50), IDSelectorNot(IDSelectorBatch([3, 5])))
    for tree in (IDSelectorGroups(group_keys[:3]), IDSelectorNot(IDSelectorGroups(group_keys[:3])),
                 IDSelectorAnd(IDSelectorRange(0, 100), IDSelectorXOr(IDSelectorAll(), IDSelectorGroups(group_keys[2:5])))):
        first = tree.resolve(ix)
        assert first.version == ix.version and tree.resolve(ix) is first
        # set_groups again over the same rows: same count, same ids array, no removal — only the version tells
        ix.version += 1
        rng_gid = np.random.default_rng(5).integers(0, 9, 200)
        ix.tables = dict(ix.tables, gid=torch.from_numpy(rng_gid.astype(np.int32)))
        second = tree.resolve(ix)
        assert second is not first and second.version == ix.version
        assert np.array_equal(_w(second.bitmap), ref.words(ref.mask(tree, ix.ids.numpy(), ix.id_base, 200, rng_gid, group_keys)))
        ix.tables = dict(ix.tables, gid=torch.from_numpy(gid.astype(np.int32)))
    before = plain.resolve(ix)
    assert before.version is None
    ix.version += 1                                                                    # a tree without a group selector does not care
    assert plain.resolve(ix) is before
    ix._mutations += 1                                                                 # ... but the keys of before still hold
    assert plain.resolve(ix) is not before
    # stale tables are never used: the index is asked on every resolution, and its RuntimeError comes through
    sel = IDSelectorGroups(group_keys[:2])
    sel.resolve(ix)
    asked = ix.asked
    sel.resolve(ix)
    assert ix.asked > asked
    ix.tables = None
    for tree in (sel, IDSelectorAnd(IDSelectorAll(), sel)):
        with pytest.raises(RuntimeError, match="set_groups"):
            tree.resolve(ix)


# --------------------------------------------------------------------------------------------------------------------- refusals
def test_group_selector_refusals_need_no_device():
    from wise_amd.index import sharded
    from wise_amd.index.flat_ip import FlatIPIndex
    from wise_amd.index.flat_pq import FlatPQIPIndex, FlatPQRefineIPIndex
    from wise_amd.index.ivf_flat import IVFFlatIPIndex, IVFFlatL2Index
    from wise_amd.index.ivf_pq import IVFOPQIPIndex, IVFPQIPIndex, IVFPQRefineIPIndex
    sel = IDSelectorGroups([1, 2])
    for pq in (IVFPQIPIndex(32, 4, 8, device="cpu"), IVFPQRefineIPIndex(32, 4, 8, 8, device="cpu"), IVFOPQIPIndex(32, 4, 8, device="cpu"),
               FlatPQIPIndex(32, 8, device="cpu"), FlatPQRefineIPIndex(32, 8, 8, device="cpu")):
        with pytest.raises(NotImplementedError, match="search_grouped is not implemented — the scores of the product-quantized"):
            sel.resolve(pq)                                                             # the NotImplementedError of set_groups
        with pytest.raises(NotImplementedError, match="product-quantized"):
            pq.set_groups([1], [1])
    for sh in (sharded.ShardedFlatIPIndex(FlatIPIndex(16, device="cpu")), sharded.ShardedIVFFlatIPIndex(IVFFlatIPIndex(16, 4, device="cpu"))):
        with pytest.raises(NotImplementedError, match="search_grouped is not implemented on a sharded index"):
            sel.resolve(sh)
        with pytest.raises(NotImplementedError):                                        # and the wrapper still takes no selector at all
            sh.search(np.zeros((1, 16), np.float32), 3, params=SearchParameters(sel=sel))
    part = IVFFlatL2Index(16, 4, device="cpu")
    part.pos_base = 128
    with pytest.raises(NotImplementedError, match=r"slice of a sharded index \(pos_base = 128\)"):
        sel.resolve(part)
    # no tables for the present rows: the RuntimeError of search_grouped, before anything is launched
    x = np.random.default_rng(0).standard_normal((10, 16)).astype(np.float32)
    ix = FlatIPIndex(16, device="cpu")
    ix.add_with_ids(x, np.arange(10))
    for tree in (sel, IDSelectorNot(sel), IDSelectorAnd(IDSelectorRange(0, 5), sel)):
        with pytest.raises(RuntimeError, match=r"call set_groups\(ids, keys\) first"):
            tree.resolve(ix)
    ix.set_groups(np.arange(10), np.arange(10) // 3)
    ix.add_with_ids(x, np.arange(10, 20))                                               # the rows changed: the tables are dropped
    with pytest.raises(RuntimeError, match="set_groups"):
        sel.resolve(ix)
    with pytest.raises(RuntimeError, match="set_groups"):
        ix.remove_ids(sel)


# ----------------------------------------------------------------------------------------------------------------- WISE surface
class _RecordingIndex:
    def __init__(self):
        self.calls = []

    def _record(self, name, args, kwargs, out):
        self.calls.append((name, args, kwargs))
        return out

    def search(self, *args, **kwargs):
        nq, k = np.asarray(args[0]).shape[0], args[1]
        return self._record("search", args, kwargs, (np.zeros((nq, k), np.float32), np.zeros((nq, k), np.int64)))

    def range_search(self, *args, **kwargs):
        return self._record("range_search", args, kwargs, (np.array([0, 0]), np.zeros(0, np.float32), np.zeros(0, np.int64)))

    def search_grouped(self, *args, **kwargs):
        nq, k = np.asarray(args[0]).shape[0], args[1]
        return self._record("search_grouped", args, kwargs, (np.zeros((nq, k), np.float32),) + (np.zeros((nq, k), np.int64),) * 2)


class _TextTower:
    def extract_text_features(self, texts):
        return np.ones((len(texts), 8), np.float32)


def test_within_groups_plumbing():
    from wise_amd.index.feature_search_index import FeatureSearchIndex
    rec = _RecordingIndex()
    si = FeatureSearchIndex("video", "extractor", {"features_dir": "f", "index_dir": "i"})
    si.index, si.feature_extractor = rec, _TextTower()
    # neither argument: today's calls exactly
    si.search("video", "dog", topk=7)
    si.search("video", "dog", topk=7, within=None, within_groups=None)
    si.search_batch("video", ["dog", "cat"], topk=7, within_groups=None)
    for name, args, kwargs in rec.calls:
        assert name == "search" and len(args) == 2 and args[1] == 7 and kwargs == {}    # positional search(q, topk), no params
    rec.calls.clear()
    si.search_range("video", "dog", 0.5)
    si.search_grouped("video", "dog", topk=3)
    assert [(name, len(args), kwargs) for name, args, kwargs in rec.calls] == [("range_search", 2, {"params": None}), ("search_grouped", 2, {"params": None})]
    # within_groups alone: an IDSelectorGroups of the keys
    rec.calls.clear()
    si.search("video", "dog", topk=4, within_groups=[9, 9, 2])
    si.search_range("video", "dog", 0.5, within_groups=np.array([9, 2]))
    si.search_grouped("video", "dog", topk=4, within_groups=(2,))
    si.search_batch("video", ["dog", "cat", "owl"], topk=4, within_groups=[2, 9])
    assert [name for name, _, _ in rec.calls] == ["search", "range_search", "search_grouped", "search"]
    for (name, args, kwargs), keys in zip(rec.calls, ([9, 9, 2], [9, 2], [2], [2, 9])):
        assert set(kwargs) == {"params"} and type(kwargs["params"]) is SearchParameters and len(args) == 2
        assert type(kwargs["params"].sel) is IDSelectorGroups and kwargs["params"].sel.keys.tolist() == keys
    assert rec.calls[3][1][0].shape == (3, 8)                                           # one batched search, one selector for all queries
    # both: the IDSelectorAnd of the two
    rec.calls.clear()
    rng_sel = IDSelectorRange(0, 10)
    si.search("video", "dog", topk=4, within=rng_sel, within_groups=[5])
    si.search_range("video", "dog", 0.5, within=[1, 2, 2], within_groups=[5])
    si.search_grouped("video", "dog", within=rng_sel, within_groups=[5])
    si.search_batch("video", ["dog"], within=[3], within_groups=[5])
    assert len(rec.calls) == 4
    for name, args, kwargs in rec.calls:
        sel = kwargs["params"].sel
        assert type(sel) is IDSelectorAnd and type(sel.rhs) is IDSelectorGroups and sel.rhs.keys.tolist() == [5]
    assert rec.calls[0][2]["params"].sel.lhs is rng_sel and rec.calls[1][2]["params"].sel.lhs.ids.tolist() == [1, 2, 2]
    # within alone stays what it was
    rec.calls.clear()
    si.search("video", "dog", within=rng_sel)
    assert rec.calls[0][2]["params"].sel is rng_sel
    with pytest.raises(TypeError):
        si.search("video", "dog", 4, "text", None, [5])                                 # keyword-only
    with pytest.raises(ValueError):
        si.search("video", "dog", within_groups=[0.5])
    assert within_selector() is None and within_selector(rng_sel) is rng_sel and type(within_selector([1])) is IDSelectorBatch
    with pytest.raises(ValueError):                                                     # a resolved `within` belongs to one index: not joined
        within_selector(ResolvedSelector(torch.zeros(1, dtype=torch.int32), 5), [1])
    assert "groups set on the loaded index" in FeatureSearchIndex.remove_groups.__doc__.lower()


def test_remove_groups_needs_a_loaded_index_with_groups(tmp_path):
    from wise_amd.index.feature_search_index import FeatureSearchIndex
    si = FeatureSearchIndex("video", "extractor", {"features_dir": str(tmp_path), "index_dir": str(tmp_path)})
    with pytest.raises(NotImplementedError):
        si.remove_groups("IndexNoSuchType", [1])
    with pytest.raises(RuntimeError, match="load_index and set_groups first"):
        si.remove_groups("IndexFlatIP", [1])
    si.index = object()
    with pytest.raises(FileNotFoundError):
        si.remove_groups("IndexFlatIP", [1])


# ----------------------------------------------------------------------------------------------------------------- declarations
def test_symbols_declared_and_bound():
    from wise_amd import _lib, build
    declared = build.declared_symbols()
    header = (ROOT / "include" / "wise_hip.h").read_text()
    for name, nargs in SYMBOLS.items():
        assert name in declared and name in _lib.SIGNATURES, name
        decl = re.search(r"^(?:int|size_t) " + name + r"\(([^;]*)\);", header, re.M | re.S)
        assert decl and len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == nargs, name
    assert set(_lib.SIGNATURES) == set(declared)
    assert "sel_tree.hip" in build.HIP_SOURCES and (build.CSRC / "sel_tree.hip").exists()
    intro = header[header.index("/* ABI version of this header"):header.index("int wise_abi_version(void);")]
    assert "The version is 5." in intro and not re.search(r"\b6:", intro)               # additive: listed as added within 5
    for name in ("wise_sel_bitmap_groups", "wise_sel_groups_workspace_bytes", "wise_sel_bitmap_idbits", "wise_sel_combine"):
        assert name in intro, name
    assert re.search(r"wise_abi_version\(void\)\s*\{\s*return 5;", (ROOT / "wise_amd" / "csrc" / "common.hip").read_text())
    flat = re.sub(r"\s*\n \*\s*", " ", header)                                         # comment text, however it is wrapped
    for phrase in ("the bits past N are zero, also when inverted", "0 <= N < 2^32 - 1", "0 <= G <= 2^31 - 1", "out may be a or b",
                   "3: a AND NOT b", "(i >> 3) < n_bytes"):                              # limits where the entries are declared
        assert phrase in flat, phrase
    integration = (ROOT / "INTEGRATION.md").read_text()
    for name in SYMBOLS:
        assert name in integration, name
    # the kernels of ivf_select.hip are not part of this: wise_sel_bitmap keeps its signature
    assert len(_lib.SIGNATURES["wise_sel_bitmap"][1]) == 11 and len(_lib.SIGNATURES["wise_sel_positions"][1]) == 8


def test_argument_rules_answer_without_a_device():
    from wise_amd import _lib
    assert _lib.LIB_PATH.exists(), "the library is not built"
    lib = _lib.load()
    assert lib.wise_abi_version() == 5
    p, E = 1 << 20, -1                                                                  # an aligned non-null address nothing reads
    assert lib.wise_sel_groups_workspace_bytes(0) == 256 and lib.wise_sel_groups_workspace_bytes(1) == 256
    assert lib.wise_sel_groups_workspace_bytes(2048) == 256 and lib.wise_sel_groups_workspace_bytes(2049) == 512
    assert lib.wise_sel_groups_workspace_bytes(50_000) == 6400 and lib.wise_sel_groups_workspace_bytes(0x7FFFFFFF) == 1 << 28
    assert lib.wise_sel_groups_workspace_bytes(-1) == 0 and lib.wise_sel_groups_workspace_bytes(0x80000000) == 0
    good = [p, 10, p, 4, p, 2, 0, p, p, 256, 0]                                         # gid N keys G sel n_sel invert bitmap ws bytes stream
    for at, val, word in ((1, -1, b"N="), (1, 0xFFFFFFFF, b"N="), (3, -1, b"G="), (3, 0x80000000, b"G="), (5, -1, b"n_sel="),
                          (0, 0, b"null gid"), (7, 0, b"null gid or bitmap"), (2, 0, b"null group_keys"), (4, 0, b"null sel_keys"),
                          (8, 0, b"workspace"), (9, 255, b"workspace 255 < 256"), (9, 0, b"workspace")):
        args = list(good)
        args[at] = val
        assert lib.wise_sel_bitmap_groups(*args) == E and word in lib.wise_last_error(), (at, val, lib.wise_last_error())
    assert lib.wise_sel_bitmap_groups(p, 10, p, 2049, p, 2, 0, p, p, 256, 0) == E and b"256 < 512" in lib.wise_last_error()
    good = [p, 0, 10, p, 4, 0, p, 0]                                                    # ids id_base N bits n_bytes invert bitmap stream
    for at, val, word in ((2, -1, b"N="), (2, 0xFFFFFFFF, b"N="), (4, -1, b"n_bytes="), (6, 0, b"null bitmap"), (3, 0, b"null bits")):
        args = list(good)
        args[at] = val
        assert lib.wise_sel_bitmap_idbits(*args) == E and word in lib.wise_last_error(), (at, val)
    good = [p, p, 10, 0, p, 0]                                                          # a b N op out stream
    for at, val, word in ((2, -1, b"N="), (2, 0xFFFFFFFF, b"N="), (3, 5, b"op=5"), (3, -1, b"op=-1"), (0, 0, b"null"), (4, 0, b"null"),
                          (1, 0, b"null")):
        args = list(good)
        args[at] = val
        assert lib.wise_sel_combine(*args) == E and word in lib.wise_last_error(), (at, val)
    # no rows: legal, nothing is launched and no pointer is looked at — also without a device
    assert lib.wise_sel_bitmap_groups(0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0) == 0
    assert lib.wise_sel_bitmap_idbits(0, 0, 0, 0, 0, 0, 0, 0) == 0
    for op in range(5):
        assert lib.wise_sel_combine(0, 0, 0, op, 0, 0) == 0
    assert lib.wise_sel_combine(0, 0, 0, 7, 0, 0) == E                                  # ... but an unknown op is still one

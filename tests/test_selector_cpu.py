"""The host side of a search restricted to a set of ids (wise_amd/index/selector.py) — what needs no GPU: the numpy restatement
the GPU tests hold the kernels to (tests/sel_ref.py), the parameter objects, the WISE-level `within` argument, the sharded
wrappers' refusal, and the declarations of the new entry points."""
import re
from pathlib import Path

import numpy as np
import pytest

import sel_ref
from wise_amd.index.selector import (IDSelector, IDSelectorBatch, IDSelectorNot, IDSelectorRange, ResolvedSelector, SearchParameters,
                                     SearchParametersIVF, as_selector, resolve_for, unpack_params)

ROOT = Path(__file__).resolve().parent.parent


# ---------------------------------------------------------------------------------------------------------------- sel_ref.resolve
def test_resolve_batch_duplicates_absent_ids_and_empty():
    ids = np.array([11, 5, 8, 300, -4, 7, 5000000000], dtype=np.int64)       # external ids by position, any order
    assert sel_ref.resolve(ids, IDSelectorBatch([8, 8, 5, 8])).tolist() == [False, True, True, False, False, False, False]
    assert sel_ref.resolve(ids, IDSelectorBatch([1, 2, 3, 9999])).tolist() == [False] * 7      # ids no row carries select nothing
    assert sel_ref.resolve(ids, IDSelectorBatch([])).tolist() == [False] * 7
    assert sel_ref.resolve(ids, IDSelectorBatch([9999, -4, 5000000000])).tolist() == [False, False, False, False, True, False, True]
    assert sel_ref.resolve(np.empty(0, np.int64), IDSelectorBatch([1])).shape == (0,)


def test_resolve_range_and_not():
    ids = np.arange(100, dtype=np.int64) * 3 + 11
    assert sel_ref.resolve(ids, IDSelectorRange(11, 11)).sum() == 0                    # empty
    assert sel_ref.resolve(ids, IDSelectorRange(50, 20)).sum() == 0                    # imax < imin: empty
    assert sel_ref.resolve(ids, IDSelectorRange(-10, 10 ** 12)).all()                  # covers all rows
    half = sel_ref.resolve(ids, IDSelectorRange(11, 11 + 3 * 50))                      # imin <= id < imax
    assert half[:50].all() and not half[50:].any()
    for s in (IDSelectorBatch([11, 14, 14, 2]), IDSelectorRange(20, 200)):
        m = sel_ref.resolve(ids, s)
        assert np.array_equal(sel_ref.resolve(ids, IDSelectorNot(s)), ~m)
        assert np.array_equal(sel_ref.resolve(ids, IDSelectorNot(IDSelectorNot(s))), m)            # Not(Not(s)) is s


def test_bitmap_layout_and_filtered_topk():
    mask = np.zeros(70, dtype=bool)
    mask[[0, 31, 32, 69]] = True
    assert sel_ref.bitmap(mask).tolist() == [0x80000001, 1, 1 << 5]                   # bit p & 31 of word p >> 5, zero tail
    assert sel_ref.bitmap(np.ones(33, bool)).tolist() == [0xFFFFFFFF, 1]
    assert sel_ref.bitmap(np.zeros(0, bool)).shape == (0,)
    # (-score, position) over the masked rows, ids looked up by position, padding at the tail
    scores = np.array([[1.0, 3.0, 3.0, 2.0, 9.0]], dtype=np.float32)
    ids = np.array([50, 40, 30, 20, 10])
    D, I, P = sel_ref.filtered_topk(scores, np.arange(5), np.array([1, 1, 1, 1, 0], bool), ids, 3)
    assert I.tolist() == [[40, 30, 20]] and P.tolist() == [[1, 2, 3]] and D.tolist() == [[3.0, 3.0, 2.0]]
    D, I, P = sel_ref.filtered_topk(scores, np.arange(5), np.array([0, 0, 0, 1, 0], bool), None, 3)
    assert I.tolist() == [[3, -1, -1]] and D[0, 0] == 2.0 and (D[0, 1:] == sel_ref.NEG).all()
    D, I, P = sel_ref.filtered_topk(scores, np.arange(5), np.zeros(5, bool), ids, 2)
    assert (I == -1).all() and (D == sel_ref.NEG).all()


def test_pq_scan_is_the_masked_prefix_of_the_full_scan():
    import ivfpq_ref
    rng = np.random.default_rng(3)
    list_off = np.array([0, 40, 40, 100, 130], dtype=np.int64)
    codes = rng.integers(0, 256, (130, 4)).astype(np.uint8)
    codes[50:60] = codes[45]                                                           # exact ties
    lut = rng.standard_normal((2, 4, 256)).astype(np.float32)
    probes = np.array([[2, -1, 0], [1, 3, -1]], dtype=np.int64)
    bias = rng.standard_normal((2, 3)).astype(np.float32)
    ids = rng.permutation(130).astype(np.int64) + 7
    full = ivfpq_ref.scan(codes, list_off, ids, lut, probes, bias, 100)
    allrows = sel_ref.pq_scan(codes, list_off, ids, lut, probes, bias, 100, np.ones(130, bool))
    assert np.array_equal(full[0].view(np.uint32), allrows[0].view(np.uint32)) and np.array_equal(full[1], allrows[1])
    mask = rng.random(130) < 0.3
    D, I = sel_ref.pq_scan(codes, list_off, ids, lut, probes, bias, 5, mask)
    for q in range(2):
        want = [(s, i) for s, i in zip(full[0][q], full[1][q]) if i >= 0 and mask[np.flatnonzero(ids == i)[0]]][:5]
        assert [i for _, i in want] == I[q, :len(want)].tolist() and (I[q, len(want):] == -1).all()
        assert np.array_equal(np.array([s for s, _ in want], np.float32).view(np.uint32), D[q, :len(want)].view(np.uint32))


class _Sel:
    """a selector as far as sel_ref.resolve reads it, from sel_ref.flat_selector_spec"""

    def __init__(self, kind, args):
        if kind == "range":
            self.imin, self.imax = args
        elif kind == "batch":
            self.ids = np.asarray(args[0], dtype=np.int64)
        else:
            self.sel = _Sel("batch", args)


@pytest.mark.parametrize("N,d", [(1000, 64), (1000, 512), (1000, 768), (4096, 64), (4096, 512), (4096, 768), (300000, 64)])
def test_flat_cases_leave_out_at_most_one_percent_of_their_ranks(N, d):
    """The near-tie rule of the flat GPU test on the oracle's own score gaps, for the seeds in sel_ref.FLAT_SEEDS (the GPU test
    asserts the same share, for (300000, 512) and (300000, 768) too)."""
    X, Q, ids = sel_ref.flat_case(N, d)
    S = sel_ref.scores_f64(X, Q)
    for which in sel_ref.SELECTIVITIES:
        mask = sel_ref.resolve(ids, _Sel(*sel_ref.flat_selector_spec(ids, which)))
        for nq in (1, 8):
            for k in (1, 10, 100):
                valid = min(k, int(mask.sum())) * nq
                assert sel_ref.near_tie_ranks(S[:nq], mask, k).sum() <= 0.01 * valid, (which, nq, k)


# ------------------------------------------------------------------------------------------------------------ parameter objects
def test_selectors_and_parameter_objects_validate():
    b = IDSelectorBatch(np.array([[3, 1], [3, 2]]))
    assert b.ids.dtype == np.int64 and b.ids.tolist() == [3, 1, 3, 2]                  # flattened, duplicates kept as given
    assert IDSelectorBatch([]).ids.shape == (0,)
    r = IDSelectorRange(5, 9)
    assert (r.imin, r.imax) == (5, 9) and IDSelectorNot(r).sel is r
    with pytest.raises(ValueError):
        IDSelectorBatch([1.5, 2.0])
    with pytest.raises(ValueError):
        IDSelectorRange(0.0, 5)
    with pytest.raises(ValueError):
        IDSelectorNot([1, 2, 3])
    assert SearchParameters().sel is None and SearchParameters(sel=b).sel is b
    p = SearchParametersIVF(sel=r, nprobe=16)
    assert p.sel is r and p.nprobe == 16 and isinstance(p, SearchParameters) and SearchParametersIVF().nprobe is None
    for bad in (0, -3, 2.5, "8", True):
        with pytest.raises(ValueError):
            SearchParametersIVF(nprobe=bad)
    with pytest.raises(ValueError):
        SearchParameters(sel=[1, 2, 3])                                                # an id list is not a selector here
    # what the index classes make of `params`
    assert unpack_params(None, ivf=False) == (None, None) and unpack_params(None, ivf=True) == (None, None)
    assert unpack_params(SearchParameters(sel=b), ivf=True) == (b, None)
    assert unpack_params(p, ivf=True) == (r, 16)
    assert unpack_params(SearchParametersIVF(sel=b), ivf=False) == (b, None)
    with pytest.raises(ValueError):
        unpack_params(p, ivf=False)                                                    # nprobe on a flat index
    for bad in ({"sel": b}, b, 5):
        with pytest.raises(ValueError):
            unpack_params(bad, ivf=True)                                               # unknown params types
    assert as_selector(r) is r and as_selector([4, 5]).ids.tolist() == [4, 5]


class _Rows:
    """an index as far as selector resolution looks at it"""
    device = "cpu"

    def __init__(self, n):
        self.n = n

    def _selector_rows(self):
        return None, 0, self.n


def test_a_selector_resolved_against_other_rows_is_refused():
    import torch
    res = ResolvedSelector(torch.zeros(4, dtype=torch.int32), 100)
    assert resolve_for(_Rows(100), None) is None
    assert resolve_for(_Rows(100), res) is res
    with pytest.raises(ValueError, match="resolved against 100 rows"):
        resolve_for(_Rows(101), res)
    with pytest.raises(ValueError):
        resolve_for(_Rows(100), [1, 2, 3])
    assert isinstance(IDSelectorBatch([1]), IDSelector)


# ----------------------------------------------------------------------------------------------------------------- WISE surface
class _RecordingIndex:
    def __init__(self):
        self.calls = []

    def search(self, *args, **kwargs):
        self.calls.append((args, kwargs))
        nq, k = np.asarray(args[0]).shape[0], args[1]
        return np.zeros((nq, k), np.float32), np.zeros((nq, k), np.int64)


class _OldIndex:
    """a test double written before `params` existed: search(x, k) and nothing else"""

    def search(self, x, k):
        return np.zeros((len(x), k), np.float32), np.arange(len(x) * k, dtype=np.int64).reshape(len(x), k)


class _TextTower:
    def extract_text_features(self, texts):
        return np.ones((len(texts), 8), np.float32)


def _search_index(index):
    from wise_amd.index.feature_search_index import FeatureSearchIndex
    si = FeatureSearchIndex("video", "extractor", {"features_dir": "f", "index_dir": "i"})
    si.index, si.feature_extractor = index, _TextTower()
    return si


def test_feature_search_index_within():
    rec = _RecordingIndex()
    si = _search_index(rec)
    si.search("video", "dog", topk=7)
    si.search("video", "dog", topk=7, within=None)
    for args, kwargs in rec.calls:                                # today's call exactly: index.search(q, topk), positional
        assert len(args) == 2 and args[1] == 7 and kwargs == {}
    dist, ids = _search_index(_OldIndex()).search("video", "dog", topk=3, within=None)
    assert ids.tolist() == [0, 1, 2]
    assert len(_search_index(_OldIndex()).search_batch("video", ["a", "b"], topk=3)) == 2
    rec.calls.clear()
    sel = IDSelectorRange(0, 10)
    si.search("video", "dog", topk=4, within=sel)
    si.search("video", "dog", topk=4, within=[5, 9, 9])
    si.search_batch("video", ["dog", "cat", "owl"], topk=4, within=np.array([1, 2]))
    assert len(rec.calls) == 3
    (a0, k0), (a1, k1), (a2, k2) = rec.calls
    assert all(len(a) == 2 and a[1] == 4 and set(k) == {"params"} and type(k["params"]) is SearchParameters for a, k in rec.calls)
    assert k0["params"].sel is sel
    assert isinstance(k1["params"].sel, IDSelectorBatch) and k1["params"].sel.ids.tolist() == [5, 9, 9]
    assert k2["params"].sel.ids.tolist() == [1, 2] and a2[0].shape == (3, 8)
    with pytest.raises(TypeError):
        si.search("video", "dog", 4, "text", sel)                 # keyword-only


def test_sharded_wrappers_refuse_a_selector():
    import torch
    from wise_amd.index.sharded import (ShardedFlatIPIndex, ShardedIVFFlatIPIndex, ShardedIVFPQIPIndex, ShardedIVFPQRefineIPIndex)

    class Local:
        d, device, nprobe, ntotal = 8, torch.device("cpu"), 4, 0
        seen = []

        def search_device(self, q, k):
            self.seen.append(self.nprobe)
            return torch.zeros(q.shape[0], k), torch.zeros(q.shape[0], k, dtype=torch.int64)

        search_local_device = search_device

    sel = IDSelectorBatch([1, 2])
    q = np.zeros((2, 8), np.float32)
    for cls in (ShardedFlatIPIndex, ShardedIVFFlatIPIndex, ShardedIVFPQIPIndex, ShardedIVFPQRefineIPIndex):
        local = Local()
        sh = cls(local)
        with pytest.raises(NotImplementedError, match="each rank would resolve"):
            sh.search(q, 3, params=SearchParameters(sel=sel))
        with pytest.raises(NotImplementedError, match="collective filtered search"):
            sh.search_device(torch.from_numpy(q), 3, sel=sel)
        with pytest.raises(ValueError):
            sh.search(q, 3, params={"sel": sel})
        D, I = sh.search(q, 3)                                    # and without one they search as before
        assert D.shape == (2, 3)
        D, I = sh.search(q, 3, params=SearchParametersIVF(nprobe=9))          # nprobe: for that call only
        assert local.seen[-1] == 9 and local.nprobe == 4


# ---------------------------------------------------------------------------------------------------------------- declarations
NEW_SYMBOLS = {"wise_sel_bitmap": 11, "wise_sel_positions_workspace_bytes": 1, "wise_sel_positions": 8, "wise_ip_topk_pos_f32": 15,
               "wise_ivf_scan_sel_f32": 17, "wise_ivfpq_scan_sel": 18}


def test_header_and_binding_declare_the_selector_entry_points():
    from wise_amd import _lib
    from wise_amd.build import HIP_SOURCES, declared_symbols

    header = (ROOT / "include" / "wise_hip.h").read_text()
    declared = declared_symbols()
    for name, nargs in NEW_SYMBOLS.items():
        assert name in declared, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"^(?:int|size_t) " + name + r"\(([^;]*)\);", header, re.M | re.S)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    # the unfiltered entry points keep their signatures, and the ABI number stays: the change is additive
    assert len(_lib.SIGNATURES["wise_ip_topk_f32"][1]) == 13 and len(_lib.SIGNATURES["wise_ivf_scan_f32"][1]) == 16
    assert len(_lib.SIGNATURES["wise_ivfpq_scan"][1]) == 17
    assert re.search(r"5: wise_ip_shadow_i8", header) and not re.search(r"\b6: ", header.split("int wise_abi_version(void);")[0])
    assert re.search(r"wise_abi_version\(void\)\s*\{\s*return 5;", (ROOT / "wise_amd" / "csrc" / "common.hip").read_text())
    assert "ivf_select.hip" in HIP_SOURCES
    # limits, ties and padding are spelled out where the entries are declared
    for phrase in ("the bits past N are zero", "the lower position wins", "n_pos == 0\n *     gives all padding",
                   "bit for bit the unfiltered scan's score"):
        assert phrase in header, phrase

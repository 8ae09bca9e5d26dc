"""No GPU: search_grouped's host side — the group tables (group_search.build_group_tables) and their ValueErrors, tests/group_ref.py
against a plain-loop reading of the contract, the entry points declared, bound and exported under ABI 5 with the argument rules that
need no device, the refusals, the RuntimeError before set_groups and after the rows change, and FeatureSearchIndex.search_grouped
over a stand-in index."""
import re
from pathlib import Path

import numpy as np
import pytest

import group_ref as gr

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = {"wise_group_workspace_bytes": 4, "wise_ip_group_scores_f32": 8, "wise_ipsq16_group_scores": 8, "wise_ipsq8_group_scores": 9,
           "wise_l2_group_scores_f32": 8, "wise_l2sq16_group_scores": 8, "wise_ivf_group_scores_f32": 12, "wise_ivfsq_group_scores": 14,
           "wise_ivfsq16_group_scores": 13, "wise_ivfl2_group_scores": 12, "wise_group_best": 8, "wise_group_topk": 16}


def _uneven_runs(rng, N, G):
    """[N] int64: group of every row, G contiguous runs of uneven length (each at least one row)"""
    cuts = np.sort(rng.choice(np.arange(1, N), size=G - 1, replace=False)) if G > 1 else np.empty(0, dtype=np.int64)
    return np.searchsorted(cuts, np.arange(N), side="right").astype(np.int64)


def _check_tables(row_ids, keys_of_rows, tables):
    gid, group_keys, group_off, group_rows = tables
    n = len(keys_of_rows)
    assert gid.dtype == np.int32 and group_keys.dtype == np.int64 and group_off.dtype == np.int64 and group_rows.dtype == np.uint32
    assert gid.shape == (n,) and group_rows.shape == (n,) and group_off.shape == (group_keys.size + 1,)
    assert np.array_equal(group_keys, np.unique(keys_of_rows))                       # ascending, each once
    assert np.array_equal(group_keys[gid], keys_of_rows)
    assert group_off[0] == 0 and group_off[-1] == n and np.all(np.diff(group_off) >= 1)
    for g in range(group_keys.size):                                                # the rows of a group, ascending
        mine = group_rows[group_off[g]:group_off[g + 1]].astype(np.int64)
        assert np.array_equal(mine, np.flatnonzero(gid == g))


def test_build_group_tables():
    from wise_amd.index.group_search import build_group_tables
    rng = np.random.default_rng(0)
    N = 500
    stored = rng.permutation(np.arange(1000, 1000 + N)).astype(np.int64)            # ids in row order
    for G in (1, 7, N):
        of_row = _uneven_runs(rng, N, G) * 3 + 5                                    # contiguous runs, keys with gaps
        for keys_of_rows in (of_row, rng.permutation(of_row)):                      # ... and scrambled over the rows
            given = rng.permutation(N)                                              # ids listed in any order, with extra ids ignored
            ids = np.concatenate([stored[given], [5, 6]])
            keys = np.concatenate([keys_of_rows[given], [77, 78]])
            _check_tables(stored, keys_of_rows, build_group_tables(stored, 0, N, ids, keys))
    # implicit ids: id_base + row
    of_row = _uneven_runs(rng, N, 9)
    _check_tables(None, of_row, build_group_tables(None, 40, N, np.arange(40, 40 + N), of_row))
    # an id stored twice puts both rows in its group; an id listed twice with ONE key is fine
    t = build_group_tables(np.array([7, 8, 7]), 0, 3, np.array([7, 8, 8]), np.array([2, 1, 1]))
    assert t[0].tolist() == [1, 0, 1] and t[1].tolist() == [1, 2] and t[2].tolist() == [0, 1, 3] and t[3].tolist() == [1, 0, 2]
    # no rows at all
    t = build_group_tables(None, 0, 0, np.array([1]), np.array([1]))
    assert t[0].size == 0 and t[1].size == 0 and t[2].tolist() == [0] and t[3].size == 0


def test_build_group_tables_errors():
    from wise_amd.index.group_search import build_group_tables
    stored = np.array([10, 11, 12, 13])
    with pytest.raises(ValueError, match=r"stored id 12 has no group"):
        build_group_tables(stored, 0, 4, np.array([10, 11, 13]), np.array([0, 0, 1]))
    with pytest.raises(ValueError, match=r"stored id 3 has no group"):
        build_group_tables(None, 2, 4, np.array([2, 4, 5]), np.array([0, 0, 1]))  # implicit ids 2 .. 5: 3 is the first missing
    with pytest.raises(ValueError, match=r"id 11 is given two different keys"):
        build_group_tables(stored, 0, 4, np.array([10, 11, 12, 13, 11]), np.array([0, 0, 1, 1, 2]))
    with pytest.raises(ValueError, match=r"must not be negative"):
        build_group_tables(stored, 0, 4, stored, np.array([0, 0, -1, 1]))
    with pytest.raises(ValueError, match=r"same length"):
        build_group_tables(stored, 0, 4, stored, np.array([0, 0, 1]))


def test_group_ref_against_brute_force():
    rng = np.random.default_rng(1)
    for metric in ("ip", "l2"):
        for trial in range(6):
            N, nq, G = 40, 3, (1, 5, 40, 7, 12, 3)[trial]
            gid = rng.permutation(_uneven_runs(rng, N, G)) if trial % 2 else _uneven_runs(rng, N, G)
            group_keys = np.arange(G) * 2 + 1
            ids = rng.permutation(N) + 100
            scores = rng.integers(-2, 3, size=(nq, N)).astype(np.float32)           # many equal scores: the tie rule decides
            scores[0, 3] = np.float32(-0.0)
            pos = np.arange(N)
            mask = rng.random((nq, N)) < 0.6
            mask[:, gid == 0] = trial % 3 != 0                                      # a whole group without candidates
            for k in (1, 4, G + 3):
                a = gr.grouped(scores, pos, gid, group_keys, k, mask, ids, 0, metric)
                b = gr.brute_force(scores, pos, gid, group_keys, k, mask, ids, 0, metric)
                for x, y in zip(a, b):
                    assert np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)
            # a subset of the rows as candidates (the probed lists of an inverted-file index), positions in any order
            sub = rng.permutation(N)[:25]
            a = gr.grouped(scores[:, sub], sub, gid, group_keys, 6, None, None, 7, metric)
            b = gr.brute_force(scores[:, sub], sub, gid, group_keys, 6, None, None, 7, metric)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # the two stages on their own agree with the whole
    ord_ = rng.integers(0, 4, size=(2, 30)).astype(np.uint32)
    ord_ = np.where(ord_ != 0, ord_ + np.uint32(0xBF800000), 0).astype(np.uint32)  # 0, or the image of a float just above 1.0
    gid = _uneven_runs(rng, 30, 6)
    ord_[0, gid == 2] = 0                                                           # a group without a candidate
    a = gr.select(gr.best_keys(ord_, gid, 6), 7, gid, np.arange(6) + 50)
    b = gr.grouped(gr.f32_unorder(ord_), np.arange(30), gid, np.arange(6) + 50, 7, ord_ != 0)
    assert all(np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)
               for x, y in zip(a, b))
    assert 52 not in a[2][0] and a[1][0, 5] == -1 and a[2][1, 6] == -1
    # the ordered image: order-preserving, -0.0 below +0.0, and its inverse
    v = np.array([-np.inf, -3.0, -0.0, 0.0, 1e-30, 2.5, np.inf], dtype=np.float32)
    o = gr.f32_order(v)
    assert np.all(np.diff(o.astype(np.int64)) > 0) and np.array_equal(gr.f32_unorder(o).view(np.int32), v.view(np.int32))


def test_symbols_declared_and_bound():
    from wise_amd import _lib, build
    declared = build.declared_symbols()
    header = (ROOT / "include" / "wise_hip.h").read_text()
    for name, nargs in SYMBOLS.items():
        assert name in declared and name in _lib.SIGNATURES, name
        decl = re.search(r"\b(?:int|size_t) " + name + r"\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]) == nargs, name
    assert set(_lib.SIGNATURES) == set(declared)
    assert "group_topk.hip" in build.HIP_SOURCES and (build.CSRC / "group_topk.hip").exists()
    intro = header[header.index("/* ABI version of this header"):header.index("int wise_abi_version(void);")]
    assert "The version is 5." in intro and "wise_group_best" in intro and not re.search(r"\b6:", intro)
    integration = (ROOT / "INTEGRATION.md").read_text()
    for name in SYMBOLS:
        assert name in integration, name


def test_library_exports_and_argument_rules():
    from wise_amd import _lib
    if not _lib.LIB_PATH.exists():
        pytest.skip("library not built")
    lib = _lib.load()
    assert lib.wise_abi_version() == 5
    align = lambda v: (v + 255) // 256 * 256
    # ord, best and the parts, each aligned to 256 bytes: 4 N + 8 G bytes a query plus the parts
    assert lib.wise_group_workspace_bytes(5000, 700, 3, 10) == align(4 * 3 * 5000) + align(8 * 3 * 700) + align(8 * 3 * 10)
    assert lib.wise_group_workspace_bytes(0, 0, 1, 1) > 0
    one = lib.wise_group_workspace_bytes(10_000_000, 50_000, 1, 10)
    assert 40_400_000 <= one <= 40_500_000 and (256 << 20) // one == 6            # about 6 queries a chunk at 10M rows
    for bad in ((-1, 0, 1, 1), (0xFFFFFFFF, 1, 1, 1), (10, 11, 1, 1), (10, -1, 1, 1), (10, 5, 0, 1), (10, 5, 65536, 1), (10, 5, 1, 0),
                (10, 5, 1, 2049), (0xFFFFFFF0, 0x80000000, 1, 1)):                      # gid is int32: G stops at 2^31 - 1
        assert lib.wise_group_workspace_bytes(*bad) == 0, bad
    # argument checks come before any launch, and the message says which argument
    p = 1 << 20                                                                    # an aligned non-null address nothing reads
    for args, word in (((p, -1, 1, p, p, 0, p, 0), b"N="), ((p, 10, 1, p, p, 11, p, 0), b"G="), ((p, 10, 0, p, p, 5, p, 0), b"nq="),
                       ((p, 10, 1, 0, p, 5, p, 0), b"null")):
        assert lib.wise_group_best(*args) == -1 and word in lib.wise_last_error(), args
    assert lib.wise_group_workspace_bytes(0xFFFFFFF0, 0x7FFFFFFF, 1, 1) > 0
    assert lib.wise_group_best(p, 0xFFFFFFF0, 1, p, p, 0x80000000, p, 0) == -1 and b"G=" in lib.wise_last_error()
    ok = (p, 5, 1, 10, p, 10, p, 0, 0, 0, p, p, p, p, 1 << 20, 0)
    for at, val, word in ((1, 11, b"G="), (2, 0, b"nq="), (3, 0, b"k="), (3, 2049, b"k="), (5, 0xFFFFFFFF, b"N="), (10, 0, b"null"),
                          (14, 8, b"workspace")):
        args = list(ok)
        args[at] = val
        assert lib.wise_group_topk(*args) == -1 and word in lib.wise_last_error(), (at, val)
    assert lib.wise_ip_group_scores_f32(p, 10, 6, p, 1, 0, p, 0) == -1 and b"d=6" in lib.wise_last_error()
    assert lib.wise_ip_group_scores_f32(p, 10, 16, p, 0, 0, p, 0) == -1 and b"nq=0" in lib.wise_last_error()
    assert lib.wise_ipsq16_group_scores(p, 10, 24, p, 1, 0, p, 0) == -1 and b"d=24" in lib.wise_last_error()
    assert lib.wise_l2_group_scores_f32(p, 0xFFFFFFFF, 16, p, 1, 0, p, 0) == -1 and b"N=" in lib.wise_last_error()
    assert lib.wise_l2sq16_group_scores(p, 10, 16, p + 4, 1, 0, p, 0) == -1 and b"aligned" in lib.wise_last_error()
    assert lib.wise_ipsq8_group_scores(p, 10, 16, p, 0, 1, 0, p, 0) == -1 and b"q0" in lib.wise_last_error()
    assert lib.wise_ivf_group_scores_f32(p, 10, 16, p, 2, p, 1, p, 2049, 0, p, 0) == -1 and b"nprobe=2049" in lib.wise_last_error()
    assert lib.wise_ivfsq_group_scores(p, 10, 16, p, 2, p, 0, 1, p, p, 1, 0, p, 0) == -1 and b"null" in lib.wise_last_error()
    assert lib.wise_ivfsq16_group_scores(p, 10, 16, p, 0, p, 1, p, p, 1, 0, p, 0) == -1 and b"nlist=0" in lib.wise_last_error()
    assert lib.wise_ivfl2_group_scores(p, 10, 20, p, 2, p, 1, p, 1, 0, p, 0) == -1 and b"d=20" in lib.wise_last_error()


def test_refusals_need_no_device():
    from wise_amd.index import group_search as gs
    from wise_amd.index.flat_ip import FlatIPIndex
    from wise_amd.index.flat_pq import FlatPQIPIndex, FlatPQRefineIPIndex
    from wise_amd.index.ivf_flat import IVFFlatIPIndex, IVFFlatL2Index
    from wise_amd.index.ivf_pq import IVFOPQIPIndex, IVFPQIPIndex, IVFPQRefineIPIndex
    from wise_amd.index.ivf_sq import IVFSQIPIndex
    from wise_amd.index import sharded
    x = np.zeros((1, 32), dtype=np.float32)
    for pq in (IVFPQIPIndex(32, 4, 8, device="cpu"), IVFPQRefineIPIndex(32, 4, 8, 8, device="cpu"), IVFOPQIPIndex(32, 4, 8, device="cpu"),
               FlatPQIPIndex(32, 8, device="cpu"), FlatPQRefineIPIndex(32, 8, 8, device="cpu")):
        for call in (lambda: pq.search_grouped(x, 3), lambda: pq.set_groups([1], [1]), lambda: pq.search_grouped_device(None, 3)):
            with pytest.raises(NotImplementedError, match="search_grouped is not implemented — the scores of the product-quantized"):
                call()
    for sh in (sharded.ShardedFlatIPIndex(FlatIPIndex(16, device="cpu")), sharded.ShardedIVFFlatIPIndex(IVFFlatIPIndex(16, 4, device="cpu")),
               sharded.ShardedIVFSQIPIndex(IVFSQIPIndex(32, 4, device="cpu"))):
        for call in (lambda: sh.search_grouped(x, 3), lambda: sh.set_groups([1], [1]), lambda: sh.search_grouped_device(None, 3)):
            with pytest.raises(NotImplementedError, match="search_grouped is not implemented on a sharded index"):
                call()
    part = IVFFlatL2Index(16, 4, device="cpu")
    part.pos_base = 128                                                             # a rank's slice of a sharded index
    with pytest.raises(NotImplementedError, match=r"slice of a sharded index \(pos_base = 128\)"):
        part.set_groups([1], [1])
    with pytest.raises(NotImplementedError, match="slice of a sharded index"):
        part.search_grouped(x[:, :16], 3)
    assert "set_groups" in gs.NO_GROUPS


def test_runtime_error_without_current_groups(monkeypatch):
    import torch
    from wise_amd.index import mutate
    from wise_amd.index.flat_ip import FlatIPIndex
    from wise_amd.index.flat_l2 import FlatL2Index
    from wise_amd.index.flat_sq import FlatSQfp16IPIndex
    from wise_amd.index.ivf_flat import IVFFlatIPIndex
    rng = np.random.default_rng(2)
    x = rng.standard_normal((10, 16)).astype(np.float32)
    for cls in (FlatIPIndex, FlatL2Index):
        ix = cls(16, device="cpu")
        assert ix.ngroups == 0
        with pytest.raises(RuntimeError, match=r"call set_groups\(ids, keys\) first"):
            ix.search_grouped(x[:1], 3)
        ix.add_with_ids(x, np.arange(100, 110))
        with pytest.raises(RuntimeError, match="set_groups"):
            ix.search_grouped(x[:1], 3)
        with pytest.raises(ValueError, match="stored id 105 has no group"):
            ix.set_groups(np.arange(100, 105), np.zeros(5))
        assert ix.ngroups == 0
        ix.set_groups(np.arange(90, 120), np.arange(30) // 4)
        assert ix.ngroups == 3                                                      # ids 100 .. 109 -> keys 2, 3, 4
        g = ix._group_tables()
        assert g["gid"].dtype == torch.int32 and g["keys"].tolist() == [2, 3, 4] and g["off"].tolist() == [0, 2, 6, 10] and g["n"] == 10
        ix.add_with_ids(x, np.arange(200, 210))                                     # the rows changed: the tables are dropped
        assert ix.ngroups == 0 and ix._groups is None
        with pytest.raises(RuntimeError, match="set_groups"):
            ix.search_grouped(x[:1], 3)
        ix.set_groups(np.arange(90, 220), np.arange(130) // 4)
        assert ix.ngroups > 0
        # remove_ids, with the device's compaction plan stood in for by one that drops the first row
        class Plan:
            n, kept = 20, 19
            rows = staticmethod(lambda t: t[1:])
        monkeypatch.setattr(mutate, "start", lambda index, sel, scratch: Plan)
        assert ix.remove_ids(np.array([100])) == 1 and ix.ntotal == 19
        assert ix.ngroups == 0
        with pytest.raises(RuntimeError, match="set_groups"):
            ix.search_grouped(x[:1], 3)
        monkeypatch.undo()
        ix.set_groups(np.arange(90, 220), np.arange(130) // 4)
        ix.clear_groups()
        assert ix.ngroups == 0
        ix.set_groups(np.arange(90, 220), np.arange(130) // 4)
        ix.adopt(torch.from_numpy(x), None, id_base=5)                              # adopted rows: implicit ids, no tables
        assert ix.ngroups == 0
        ix.set_groups(np.arange(5, 15), np.arange(10) % 2)
        assert ix.ngroups == 2 and ix._group_tables()["rows"].tolist() == [0, 2, 4, 6, 8, 1, 3, 5, 7, 9]
    h = FlatSQfp16IPIndex(16, device="cpu")
    h.add_halves_with_ids(x.astype(np.float16), np.arange(10))
    h.set_groups(np.arange(10), np.arange(10))
    assert h.ngroups == 10
    h.add_halves_with_ids(x.astype(np.float16), np.arange(10, 20))
    assert h.ngroups == 0
    # an inverted-file index: the tables go with every change of its lists
    iv = IVFFlatIPIndex(16, 4, device="cpu")
    with pytest.raises(RuntimeError, match="set_groups"):
        iv.search_grouped(x[:1], 3)
    iv.adopt_lists(torch.from_numpy(x), torch.arange(10), torch.tensor([0, 3, 3, 8, 10]))
    iv.set_groups(np.arange(10), np.arange(10) // 5)
    assert iv.ngroups == 2
    iv.adopt_lists(torch.from_numpy(x), torch.arange(10), torch.tensor([0, 3, 3, 8, 10]))
    assert iv.ngroups == 0
    with pytest.raises(RuntimeError, match="set_groups"):
        iv.search_grouped(x[:1], 3)


def test_feature_search_index_search_grouped():
    from wise_amd.index.feature_search_index import FeatureSearchIndex
    from wise_amd.index.selector import IDSelectorBatch

    class Extractor:
        def extract_text_features(self, texts):
            self.texts = list(texts)
            return np.ones((len(texts), 4), dtype=np.float32)

    class Index:
        def set_groups(self, ids, keys):
            self.groups = (list(ids), list(keys))

        def search_grouped(self, x, k, params=None):
            self.call = (x.shape, k, params)
            nq = x.shape[0]
            return (np.tile(np.arange(k, dtype=np.float32), (nq, 1)), np.tile(np.arange(k) + 10, (nq, 1)), np.tile(np.arange(k) + 100, (nq, 1)))

    si = FeatureSearchIndex.__new__(FeatureSearchIndex)
    si.index, si.feature_extractor, si.prompt = Index(), Extractor(), {"video": "a photo of ", "audio": "the sound of "}
    si.set_groups([1, 2], [7, 7])
    assert si.index.groups == ([1, 2], [7, 7])
    dist, ids, groups = si.search_grouped("video", "a dog", topk=3)
    assert si.feature_extractor.texts == ["a photo of a dog"] and si.index.call == ((1, 4), 3, None)
    assert dist.tolist() == [0, 1, 2] and ids.tolist() == [10, 11, 12] and groups.tolist() == [100, 101, 102]
    si.search_grouped("audio", "rain")                                              # a string is taken as it is, as on `search`
    assert si.feature_extractor.texts == ["rain"] and si.index.call[1] == 5
    si.search_grouped("audio", ["rain", "wind"], topk=2)
    assert si.feature_extractor.texts == ["the sound of rain", "the sound of wind"]
    si.search_grouped("video", "a dog", within=[3, 4])
    assert isinstance(si.index.call[2].sel, IDSelectorBatch)
    with pytest.raises(ValueError):
        si.search_grouped("video", "a dog", query_type="image")

"""CPU tests (-m "not gpu") of IndexFlatL2: the entry points are declared, exported and bound; the index file ('IxMp' around 'IxF2',
metric_type 1); the type's name in the plugin; the plugin surface over a numpy stand-in for FlatL2Index, in one process and at
world size 2 (gloo); the restatement against float64; the recorded error band of the batched search.  The kernels themselves:
tests/test_gpu_flat_l2.py."""
import json
import os
import re
import socket
import struct
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import l2_flat_ref as ref  # noqa: E402
from wise_amd import _lib  # noqa: E402
from wise_amd.index import faiss_io  # noqa: E402

ITYPE = "IndexFlatL2"
FID = "mlfoundations/open_clip/ViT-B-32/seeded-0"
# entry point -> number of arguments
NEW_SYMBOLS = {"wise_l2_topk_f32": 13, "wise_l2_topk_pos_f32": 15, "wise_l2_range_count_f32": 11, "wise_l2_range_fill_f32": 14,
               "wise_l2_prepare": 7, "wise_l2_topk_batched": 17}
NEW_SIZES = {"wise_l2_topk_workspace_bytes": 4, "wise_l2_range_workspace_bytes": 3, "wise_l2_topk_batched_workspace_bytes": 4}


def rows_of_mixed_length(n, d, seed):
    """rows that are NOT normalised: lengths spread over 0.2 .. 3, where L2 and the inner product rank differently"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, d)) / np.sqrt(d) * rng.uniform(0.2, 3.0, size=(n, 1))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
def test_entry_points_declared_exported_and_bound():
    from wise_amd.build import HIP_SOURCES, CSRC, declared_symbols

    declared = set(declared_symbols())
    assert set(_lib.SIGNATURES) == declared
    assert "l2_topk.hip" in HIP_SOURCES and (CSRC / "l2_topk.hip").exists() and "CodecL2" in (CSRC / "sq_codec.h").read_text()
    lib = _lib.load()
    header = (ROOT / "include" / "wise_hip.h").read_text()
    for name, nargs in NEW_SYMBOLS.items():
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
        decl = re.search(r"\bint\s+" + name + r"\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]) == nargs, name
    for name, nargs in NEW_SIZES.items():
        assert name in declared and getattr(lib, name) is not None
        decl = re.search(r"\bsize_t\s+" + name + r"\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]) == nargs, name
    assert lib.wise_abi_version() == 5
    assert "wise_l2_" in header.split("int wise_abi_version(void);")[0]              # listed as added within 5
    assert "THE DISTANCE IS A CONTRACT" in header and "THE DISTANCE IS A CONTRACT" in ref.__doc__
    integration = (ROOT / "INTEGRATION.md").read_text()
    for name in list(NEW_SYMBOLS) + list(NEW_SIZES):
        assert name in integration, name


def test_workspace_functions_answer_without_a_device():
    lib = _lib.load()
    assert lib.wise_l2_topk_workspace_bytes(1000, 64, 4, 10) > 0
    assert lib.wise_l2_topk_workspace_bytes(0, 64, 1, 10) > 0                       # an empty index is searched: all padding
    assert lib.wise_l2_topk_workspace_bytes(70001, 16, 1024, 2048) > 0 and lib.wise_l2_topk_workspace_bytes(1000, 1024, 1, 1) > 0
    for N, d, nq, k in ((1000, 20, 1, 10), (1000, 8, 1, 10), (1000, 1040, 1, 10), (1000, 64, 0, 10), (1000, 64, 1025, 10),
                        (1000, 64, 1, 0), (1000, 64, 1, 2049), (-1, 64, 1, 10), ((1 << 32) - 1, 64, 1, 10)):
        assert lib.wise_l2_topk_workspace_bytes(N, d, nq, k) == 0, (N, d, nq, k)
    assert lib.wise_l2_range_workspace_bytes(5000, 64, 3) > 0 and lib.wise_l2_range_workspace_bytes(0, 64, 3) >= 0
    for N, d, nq in ((5000, 20, 3), (5000, 64, 0), (5000, 64, 65536), (-1, 64, 3)):
        assert lib.wise_l2_range_workspace_bytes(N, d, nq) == 0, (N, d, nq)
    # the batched search: d % 128 == 0 in [256, 1024], nq >= 3, k <= 128, N >= 4096 — and NO large-N floor beyond that
    for d in (256, 512, 768, 1024):
        assert lib.wise_l2_topk_batched_workspace_bytes(4096, d, 3, 128) > 0
        assert lib.wise_l2_topk_batched_workspace_bytes(40000, d, 130, 10) > 0
    for N, d, nq, k in ((4095, 512, 64, 10), (40000, 512, 2, 10), (40000, 512, 64, 129), (40000, 128, 64, 10), (40000, 320, 64, 10),
                        (40000, 20, 64, 10), (1 << 31, 512, 64, 10), (40000, 512, 1025, 10)):
        assert lib.wise_l2_topk_batched_workspace_bytes(N, d, nq, k) == 0, (N, d, nq, k)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
@pytest.mark.parametrize("d", [16, 48, 512, 1024])
def test_restatement_equals_the_float64_distance_within_its_rounding_term(d):
    X, Q = rows_of_mixed_length(300, d, d), rows_of_mixed_length(4, d, d + 1)
    X[5] = Q[0]                                                          # a distance of exactly +0
    X[6] = Q[1] * np.float32(1.0 + 2.0 ** -20)                           # heavy cancellation in every difference
    S = ref.dists(X, Q)
    assert S.dtype == np.float32 and S[0, 5] == 0 and not np.signbit(S[0, 5]) and (S >= 0).all()
    err = np.abs(S.astype(np.float64) - ref.real_dists(X, Q))
    term = ref.rounding_term(d, Q, X)
    assert (err <= term[:, None]).all(), (err.max(), term.min())
    # the chain's order is the contract's, not numpy's: element i of chunk c is e = (i / 4) (d / 4) + 4 c + i % 4
    C = d // 16
    e = np.array([[(i // 4) * (d // 4) + 4 * c + i % 4 for i in range(16)] for c in range(C)])
    assert np.array_equal(ref.chunked(np.arange(d, dtype=np.float32)[None])[0], e.astype(np.float32))
    # selection: ascending distance, ties to the lower position, faiss's L2 padding
    X[200] = X[100]
    D, I = ref.topk(X, X[100:101], 5)
    assert I[0, :2].tolist() == [100, 200] and D[0, 0] == D[0, 1] == 0 and (np.diff(D[0]) >= 0).all()
    D, I = ref.topk(X[:3], Q, 5, id_base=7)
    assert (I[:, 3:] == -1).all() and (D[:, 3:] == np.float32(3.4028235e38)).all() and (I[:, :3] >= 7).all()
    lims, Dr, Ir = ref.range_search(X, Q, float(np.sort(S, axis=1)[:, 10].max()))
    for q in range(4):
        seg = Dr[lims[q]:lims[q + 1]]
        assert len(seg) >= 10 and (np.diff(seg) >= 0).all() and (seg < np.sort(S, axis=1)[:, 10].max()).all()


def test_recorded_error_band_of_the_batched_search():
    """eps of wise_l2_topk_batched, term by term, on the study data: observed <= bound for every term and for their sum, every row of
    the exact top-k is listed, and the longest list is far from the 4096 rows a list holds.  d = 256 is recomputed here; d = 1024
    is read from the record (python tests/l2_flat_ref.py rewrites it)."""
    gold = json.loads((ROOT / "tests" / "golden" / "flat_l2_band.json").read_text())
    assert json.dumps(ref.STUDY) in gold["what"] and [r["d"] for r in gold["runs"]] == [256, 1024]
    assert ref.STUDY["rows"] == 40000 and ref.STUDY["queries"] == 128 and ref.STUDY["k"] == 10 and ref.STUDY["sample_every"] == 16
    run = ref.band_study(256)
    assert set(run["terms"]) == {"query_rounding", "row_rounding", "accumulation", "half_norm", "contract"}
    rec = gold["runs"][0]
    assert run["longest_list"] == rec["longest_list"] and run["topk_rows_listed"] is True
    for name, t in list(run["terms"].items()) + [("total", run["total"])]:
        g = rec["terms"][name] if name != "total" else rec["total"]
        assert t["observed"] == pytest.approx(g["observed"], rel=1e-6) and t["bound"] == pytest.approx(g["bound"], rel=1e-9), name
    for r in gold["runs"] + [run]:
        for name, t in list(r["terms"].items()) + [("total", r["total"])]:
            assert 0.0 < t["observed"] <= t["bound"] and t["ratio"] <= 1.0, (r["d"], name, t)
        assert r["topk_rows_listed"] is True and r["longest_list"] < 4096 // 4, r["longest_list"]
        assert r["total"]["ratio"] < 0.5                                 # the band is not tight on benign data


# ---------------------------------------------------------------------------------------------------------------------
# the file
@pytest.mark.parametrize("n", [0, 1, 6])
def test_file_round_trip_is_byte_stable(tmp_path, n):
    d = 32
    X, ids = rows_of_mixed_length(n, d, 3), (np.arange(n, dtype=np.int64) * 7 + 5)
    fn = tmp_path / "a.faiss"
    faiss_io.write_idmap_flat_l2(fn, X, ids)
    raw = fn.read_bytes()
    # the layout, restated: 'IxMp' + header, 'IxF2' + header, both with metric_type 1, the rows, the id map
    hdr = struct.pack("<iqqq?i", d, n, 1 << 20, 1 << 20, True, 1)
    want = b"IxMp" + hdr + b"IxF2" + hdr + struct.pack("<Q", n * d) + X.tobytes() + struct.pack("<Q", n) + ids.tobytes()
    assert raw == want
    assert faiss_io.index_fourcc(fn) == "IxMp" and faiss_io.index_fourcc(fn, inner=True) == "IxF2"
    assert faiss_io.idmap_flat_l2_ntotal(fn) == n
    for mmap in (True, False):
        X2, ids2 = faiss_io.read_idmap_flat_l2(fn, mmap=mmap)
        assert X2.dtype == np.float32 and X2.shape == (n, d) and X2.tobytes() == X.tobytes() and np.array_equal(ids2, ids)
    again = tmp_path / "b.faiss"
    faiss_io.write_idmap_flat_l2(again, *faiss_io.read_idmap_flat_l2(fn))
    assert again.read_bytes() == raw
    for lo, hi in ((0, n), (n // 3, n - n // 4), (n, n)):
        Xr, idr = faiss_io.read_idmap_flat_l2_range(fn, lo, hi)
        assert Xr.tobytes() == X[lo:hi].tobytes() and np.array_equal(idr, ids[lo:hi])
    with pytest.raises(ValueError, match="outside"):
        faiss_io.read_idmap_flat_l2_range(fn, 0, n + 1)
    # the inner-product file of the same rows differs in its fourcc and its two metric fields only
    ip = tmp_path / "ip.faiss"
    faiss_io.write_idmap_flat_ip(ip, X, ids)
    a, b = ip.read_bytes(), raw
    assert len(a) == len(b) and [i for i in range(len(a)) if a[i] != b[i]] == [4 + 29, 4 + 33 + 3, 4 + 33 + 4 + 29]


def test_bare_record_reads_with_ids_equal_to_positions(tmp_path):
    n, d = 9, 16
    X = rows_of_mixed_length(n, d, 4)
    hdr = struct.pack("<iqqq?i", d, n, 1 << 20, 1 << 20, True, 1)
    fn = tmp_path / "bare.faiss"
    fn.write_bytes(b"IxF2" + hdr + struct.pack("<Q", n * d) + X.tobytes())
    X2, ids = faiss_io.read_idmap_flat_l2(fn)
    assert X2.tobytes() == X.tobytes() and np.array_equal(ids, np.arange(n))
    assert faiss_io.index_fourcc(fn) == faiss_io.index_fourcc(fn, inner=True) == "IxF2" and faiss_io.idmap_flat_l2_ntotal(fn) == n
    Xr, idr = faiss_io.read_idmap_flat_l2_range(fn, 2, 6)
    assert Xr.tobytes() == X[2:6].tobytes() and np.array_equal(idr, np.arange(2, 6))


def test_cut_files_and_metric_mismatches_are_refused_by_name(tmp_path):
    n, d = 6, 16
    X, ids = rows_of_mixed_length(n, d, 5), np.arange(n, dtype=np.int64)
    good = tmp_path / "good.faiss"
    faiss_io.write_idmap_flat_l2(good, X, ids)
    raw = good.read_bytes()
    readers = (faiss_io.read_idmap_flat_l2, faiss_io.idmap_flat_l2_ntotal, lambda p: faiss_io.read_idmap_flat_l2_range(p, 0, 1))
    for cut in (2, 8 * n, 8 * n + 8, 8 * n + 8 + 5, len(raw) - 50, len(raw) - 10):
        fn = tmp_path / f"short_{cut}.faiss"
        fn.write_bytes(raw[:len(raw) - cut])
        for call in readers[:1] + readers[2:]:
            with pytest.raises(RuntimeError, match=re.escape(str(fn))):
                call(fn)
    with pytest.raises(RuntimeError, match="No such file"):
        faiss_io.read_idmap_flat_l2(tmp_path / "missing.faiss")
    inner_metric, outer_metric = 4 + 33 + 4 + 29, 4 + 29
    cases = {
        "IxF2 with metric 0": raw[:inner_metric] + struct.pack("<i", 0) + raw[inner_metric + 4:],
        "id map with metric 0": raw[:outer_metric] + struct.pack("<i", 0) + raw[outer_metric + 4:],
        "count": raw[:4 + 33 + 4 + 33] + struct.pack("<Q", n * d - 1) + raw[4 + 33 + 4 + 33 + 8:],
        "outer d": raw[:4] + struct.pack("<i", d + 16) + raw[8:],
    }
    for what, data in cases.items():
        fn = tmp_path / ("bad_" + what.replace(" ", "_") + ".faiss")
        fn.write_bytes(data)
        for call in readers:
            with pytest.raises(RuntimeError, match=re.escape(str(fn))) as e:
                call(fn)
            if "metric" in what:
                assert "IndexFlatL2" in str(e.value) and "metric_type" in str(e.value)
    # an 'IxFI' file with metric 1 is refused by name too, by the inner-product reader
    ip = tmp_path / "ip.faiss"
    faiss_io.write_idmap_flat_ip(ip, X, ids)
    ipraw = ip.read_bytes()
    for what, at in (("inner", inner_metric), ("outer", outer_metric)):
        fn = tmp_path / f"ip_metric1_{what}.faiss"
        fn.write_bytes(ipraw[:at] + struct.pack("<i", 1) + ipraw[at + 4:])
        with pytest.raises(RuntimeError, match=re.escape(str(fn))) as e:
            faiss_io.read_idmap_flat_ip(fn)
        assert "IndexFlatIP" in str(e.value) and "metric_type" in str(e.value)
    # neither reader takes the other's file, nor the binary16 one's
    with pytest.raises(RuntimeError, match="is not IndexFlatL2"):
        faiss_io.read_idmap_flat_l2(ip)
    with pytest.raises(RuntimeError, match="expected IndexFlatIP"):
        faiss_io.read_idmap_flat_ip(good)
    with pytest.raises(RuntimeError, match="is not IndexScalarQuantizer"):
        faiss_io.read_idmap_sq16_ip(good)
    sq = tmp_path / "sq.faiss"
    faiss_io.write_idmap_sq16_ip(sq, X.astype(np.float16), ids)
    with pytest.raises(RuntimeError, match=re.escape(str(sq))):
        faiss_io.read_idmap_flat_l2(sq)


# ---------------------------------------------------------------------------------------------------------------------
# a numpy stand-in for FlatL2Index: what FeatureSearchIndex.flat_l2_index_factory must offer
def _selected(sel, ids):
    """bool [n]: the rows a selector (wise_amd/index/selector.py) selects, evaluated on the host"""
    from wise_amd.index.selector import IDSelectorBatch, IDSelectorNot, IDSelectorRange
    if isinstance(sel, IDSelectorBatch):
        return np.isin(ids, sel.ids)
    if isinstance(sel, IDSelectorRange):
        return (ids >= sel.imin) & (ids < sel.imax)
    if isinstance(sel, IDSelectorNot):
        return ~_selected(sel.sel, ids)
    raise TypeError(type(sel).__name__)


class _CpuFlatL2:
    """reserve / add_with_ids / search_device / search / range_search / remove_ids / reconstruct_batch / _selector_rows / rows_host
    and `metric` (and merge_lists for the sharded wrapper): every answer by tests/l2_flat_ref.py."""
    metric = "l2"

    def __init__(self, d):
        self.d, self.device = int(d), torch.device("cpu")
        self.X, self.ids = np.zeros((0, d), np.float32), np.zeros(0, np.int64)
        self.is_trained = True

    def reserve(self, n):
        self.reserved = int(n)

    def add_with_ids(self, x, ids):
        assert np.asarray(x).dtype == np.float32
        self.X = np.concatenate([self.X, np.asarray(x, np.float32)])
        self.ids = np.concatenate([self.ids, np.asarray(ids, np.int64)])

    @property
    def ntotal(self):
        return self.X.shape[0]

    def _selector_rows(self):
        return torch.from_numpy(self.ids), 0, self.ntotal

    def rows_host(self):
        return self.X, self.ids

    def search_device(self, q, k, sel=None):
        Q = q.numpy()
        pos = np.arange(self.ntotal) if sel is None else np.flatnonzero(_selected(sel, self.ids))
        D, I = ref.topk_pos(self.X, Q, k, pos, ids=self.ids)
        return torch.from_numpy(D), torch.from_numpy(I)

    def search(self, x, k, params=None):
        D, I = self.search_device(torch.from_numpy(np.ascontiguousarray(x, np.float32)), k, None if params is None else params.sel)
        return D.numpy(), I.numpy()

    def range_search(self, x, thresh, params=None):
        keep = None if params is None or params.sel is None else _selected(params.sel, self.ids)
        return ref.range_search(self.X, np.ascontiguousarray(x, np.float32), thresh, ids=self.ids, keep=keep)

    def remove_ids(self, sel):
        from wise_amd.index.selector import as_selector
        gone = _selected(as_selector(sel), self.ids)
        self.X, self.ids = self.X[~gone], self.ids[~gone]
        return int(gone.sum())

    def reconstruct_batch(self, want):
        out = np.full((len(want), self.d), np.nan, np.float32)
        for i, w in enumerate(want):
            hit = np.flatnonzero(self.ids == w)
            if len(hit):
                out[i] = self.X[hit[0]]
        return out

    @staticmethod
    def merge_lists(Ds, Is, k):
        """the wrapper's merge: it keeps the larger score, and is handed negated distances"""
        from oracle import ip_topk_ref
        D, I = ip_topk_ref.merge_topk(Ds.numpy(), Is.numpy(), k)
        return torch.from_numpy(D), torch.from_numpy(I)


class _FakeTextTower:
    def __init__(self, d):
        self.d = d

    def extract_text_features(self, texts):
        import zlib
        out = np.stack([np.random.default_rng(zlib.crc32(t.encode())).standard_normal(self.d) for t in texts])
        return (out / np.sqrt(self.d)).astype(np.float32)


def _write_store(fdir, X, ids, per_file=2048):
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    fdir.mkdir(parents=True)
    st = FeatureStoreFactory.create_store(FeatureStoreType.WEBDATASET, "video", str(fdir))
    st.enable_write(per_file, 20 * 1024 * 1024)
    for i, v in zip(ids, X):
        st.add(int(i), v[None])
    st.close()


def _factory(tmp_path):
    from wise_amd.index.search_index_factory import SearchIndexFactory
    return SearchIndexFactory("video", FID, {"features_dir": tmp_path / "features", "index_dir": tmp_path / "index"})


# ---------------------------------------------------------------------------------------------------------------------
# names
def test_type_name_is_in_the_plugin_table_and_in_the_refusal_text(tmp_path):
    from wise_amd.index import feature_search_index as fsi
    from wise_amd.index import sharded
    from wise_amd.index.flat_common import FlatIndexBase
    from wise_amd.index.flat_ip import FlatIPIndex
    from wise_amd.index.flat_l2 import FlatL2Index
    from wise_amd.index.selector import IDSelectorRange

    row = fsi.FLAT_TYPES[ITYPE]
    assert fsi._family(ITYPE) is None and row.fourcc == "IxF2" and row.metric == "l2" and row.dtype is np.float32
    assert fsi.FLAT_TYPES["IndexFlatIP"].metric == "ip" and fsi.FLAT_TYPES["IndexFlatIP"].dtype is np.float32
    assert fsi.FeatureSearchIndex.flat_l2_index_factory is FlatL2Index and issubclass(FlatL2Index, FlatIndexBase)
    assert FlatL2Index.metric == "l2" and FlatIPIndex.metric == "ip"
    assert "IndexFlatL2" in fsi.__doc__ and "FlatL2Index" in fsi.__doc__
    _write_store(tmp_path / "features", rows_of_mixed_length(12, 64, 9), np.arange(12) + 1)
    si = _factory(tmp_path)
    assert si.get_index_filename(ITYPE).name == "video-IndexFlatL2.faiss"
    with pytest.raises(NotImplementedError, match="IndexSQfp16, and IndexFlatL2$"):
        si.create_index("IndexFlatL1")
    with pytest.raises(FileNotFoundError, match="create_index"):
        si.update_index(ITYPE)
    _write_store(tmp_path / "b" / "features", rows_of_mixed_length(12, 40, 9), np.arange(12) + 1)
    with pytest.raises(ValueError, match="multiple of 16"):
        _factory(tmp_path / "b").create_index(ITYPE)                     # refused before a row is read
    with pytest.raises(ValueError, match="multiple of 16"):
        FlatL2Index(40, device="cpu")
    sh = sharded.ShardedFlatIPIndex(FlatL2Index(32, device="cpu"))      # the sharded wrapper keeps its three refusals
    with pytest.raises(NotImplementedError, match="no selector"):
        sh.search_device(None, 5, sel=IDSelectorRange(0, 10))
    with pytest.raises(NotImplementedError, match="collective removal is not built"):
        sh.remove_ids(np.array([1]))
    with pytest.raises(NotImplementedError):
        sh.range_search(np.zeros((1, 32), np.float32), 0.1)


def test_range_order_hook_leaves_the_inner_product_order_unchanged():
    from wise_amd.index import range_search as rs

    D = torch.tensor([0.5, -0.0, 0.0, 2.0, 0.5, 1.0, 1.0], dtype=torch.float32)
    P = torch.tensor([4, 1, 0, 3, 2, 9, 8], dtype=torch.int64)
    counts = torch.tensor([5, 2])
    assert rs.order_segments(D, P, counts).tolist() == [3, 4, 0, 2, 1, 6, 5]                   # descending, -0 below +0, ties by position
    assert rs.order_segments(D, P, counts, ascending=False).tolist() == [3, 4, 0, 2, 1, 6, 5]
    assert rs.order_segments(D.abs(), P, counts, ascending=True).tolist() == [2, 1, 4, 0, 3, 6, 5]   # distances: ascending, ties by position


# ---------------------------------------------------------------------------------------------------------------------
# the plugin in one process
def test_plugin_create_load_search_update_with_a_stand_in(tmp_path, monkeypatch):
    from wise_amd.index import feature_search_index as fsi
    from wise_amd.index.selector import IDSelectorRange

    N, d = 300, 32
    X, ids = rows_of_mixed_length(N, d, 11), np.arange(N, dtype=np.int64) * 2 + 1
    X[200] = X[10]                                                       # equal rows: the lower position wins
    _write_store(tmp_path / "features", X, ids, per_file=64)
    monkeypatch.setattr(fsi.FeatureSearchIndex, "flat_l2_index_factory", _CpuFlatL2)
    monkeypatch.setattr(fsi, "FeatureExtractorFactory", lambda fid: _FakeTextTower(d))
    si = _factory(tmp_path)
    si.create_index(ITYPE)
    fn = si.get_index_filename(ITYPE)
    assert faiss_io.index_fourcc(fn, inner=True) == "IxF2"
    Xf, idf = faiss_io.read_idmap_flat_l2(fn)
    assert Xf.tobytes() == X.tobytes() and np.array_equal(idf, ids)
    before = fn.read_bytes()
    si.create_index(ITYPE)                                               # skip-if-exists
    assert fn.read_bytes() == before
    assert si.load_index(ITYPE) is True                                  # the fourcc decides: an fp32 payload is not assumed to be IndexFlatIP
    assert type(si.index) is _CpuFlatL2 and si.index.ntotal == N and si.index.reserved == N and si.index.X.tobytes() == X.tobytes()

    tower = _FakeTextTower(d)
    q = tower.extract_text_features(["This is a photo of a dog"])
    D1, I1 = ref.topk(X, q, 7, ids=ids)
    dist_, ids_ = si.search("video", "dog", topk=7)
    assert np.array_equal(ids_, I1[0]) and np.array_equal(dist_, D1[0]) and (np.diff(dist_) >= 0).all()
    ip_order = ids[np.argsort(-(X.astype(np.float64) @ q[0].astype(np.float64)), kind="stable")[:7]]
    assert not np.array_equal(ip_order, I1[0])                           # on these rows the inner product ranks differently
    words = ["dog", "cat", "a red car", "rain"]
    Qb = tower.extract_text_features(["This is a photo of a " + w for w in words])
    Db, Ib = ref.topk(X, Qb, 5, ids=ids)
    got = si.search_batch("video", words, topk=5)
    assert len(got) == 4 and all(np.array_equal(g[0], Db[i]) and np.array_equal(g[1], Ib[i]) for i, g in enumerate(got))
    chosen = ids[5:60:3]                                                 # within: an array of ids and a selector
    Dw, Iw = ref.topk_pos(X, q, 7, np.flatnonzero(np.isin(ids, chosen)), ids=ids)
    dw, iw = si.search("video", "dog", topk=7, within=chosen)
    assert np.array_equal(iw, Iw[0]) and np.array_equal(dw, Dw[0]) and set(iw.tolist()) <= set(chosen.tolist())
    gw = si.search_batch("video", words, topk=5, within=IDSelectorRange(101, 301))
    in_range = np.flatnonzero((ids >= 101) & (ids < 301))
    Dr, Ir = ref.topk_pos(X, Qb, 5, in_range, ids=ids)
    assert all(np.array_equal(g[0], Dr[i]) and np.array_equal(g[1], Ir[i]) for i, g in enumerate(gw))
    radius = float(np.sort(ref.dists(X, q)[0])[19])                      # search_range: every row below the radius, ascending
    lims, Dg, Ig = ref.range_search(X, q, radius, ids=ids)
    assert lims[1] == 19
    dr, ir = si.search_range("video", "dog", radius)
    assert np.array_equal(dr, Dg) and np.array_equal(ir, Ig) and (np.diff(dr) >= 0).all()

    # update_index: 40 vectors leave the store, 25 new ones arrive; the file stays an 'IxF2' file
    assert si.update_index(ITYPE) == (0, 0) and fn.read_bytes() == before
    rng = np.random.default_rng(12)
    gone = np.sort(rng.permutation(N)[:40])
    stay = np.setdiff1d(np.arange(N), gone)
    newX, new_ids = rows_of_mixed_length(25, d, 13), np.arange(25, dtype=np.int64) + 5000
    import shutil
    shutil.rmtree(tmp_path / "features")
    order = rng.permutation(len(stay) + 25)                              # the store's own order: new rows anywhere
    sX, sid = np.concatenate([X[stay], newX])[order], np.concatenate([ids[stay], new_ids])[order]
    _write_store(tmp_path / "features", sX, sid, per_file=64)
    assert si.update_index(ITYPE) == (25, 40)
    assert faiss_io.index_fourcc(fn, inner=True) == "IxF2"
    X2, id2 = faiss_io.read_idmap_flat_l2(fn)
    added = sid[np.isin(sid, new_ids)]                                   # in store order, behind the kept rows in their order
    assert np.array_equal(id2, np.concatenate([ids[stay], added]))
    assert X2.tobytes() == np.concatenate([X[stay], sX[np.isin(sid, new_ids)]]).tobytes()
    assert si.update_index(ITYPE) == (0, 0)
    assert si.load_index(ITYPE) is True and si.index.ntotal == N - 40 + 25
    D3, I3 = ref.topk(np.asarray(X2), q, 7, ids=id2)
    dist3, ids3 = si.search("video", "dog", topk=7)
    assert np.array_equal(ids3, I3[0]) and np.array_equal(dist3, D3[0])
    # and IndexFlatIP beside it, same store: its file stays 'IxFI' through an update (the payload's dtype no longer names the type)
    from wise_amd.index.flat_ip import FlatIPIndex  # noqa: F401  (the class attribute the stand-in replaces)

    class _CpuFlatIP(_CpuFlatL2):
        metric = "ip"
    monkeypatch.setattr(fsi.FeatureSearchIndex, "flat_index_factory", _CpuFlatIP)
    si.create_index("IndexFlatIP")
    fip = si.get_index_filename("IndexFlatIP")
    assert faiss_io.index_fourcc(fip, inner=True) == "IxFI"
    shutil.rmtree(tmp_path / "features")
    _write_store(tmp_path / "features", sX[:-3], sid[:-3], per_file=64)
    assert si.update_index("IndexFlatIP") == (0, 3) and faiss_io.index_fourcc(fip, inner=True) == "IxFI"
    assert si.load_index("IndexFlatIP") is True and type(si.index) is _CpuFlatIP


# ---------------------------------------------------------------------------------------------------------------------
# the plugin at world size 2 (gloo): parts built from each rank's own store shards, and ranges of the single file
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


WANT_IDS = [1, 1001, 500, 1006]


def _plugin_worker(rank, world, port, root, N, d):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import wise_amd.index.feature_search_index as fsi
    from wise_amd.index.search_index_factory import SearchIndexFactory
    from wise_amd.index.selector import IDSelectorRange, SearchParameters
    from wise_amd.index.sharded import NO_SELECTOR, ShardedFlatIPIndex, shard_range

    fsi.FeatureSearchIndex.flat_l2_index_factory = _CpuFlatL2
    fsi.FeatureExtractorFactory = lambda fid: _FakeTextTower(d)
    root = Path(root)
    Q = rows_of_mixed_length(3, d, 6)
    out = {}
    si2 = SearchIndexFactory("video", FID, {"features_dir": root / "features", "index_dir": root / "index_parts"})
    si2.create_index(ITYPE)                                              # every rank reads its own tar files only and writes its own part
    part = si2.get_index_part_filename(ITYPE, rank, world)
    assert part.exists() and not si2.get_index_filename(ITYPE).exists() and faiss_io.index_fourcc(part, inner=True) == "IxF2"
    dist.barrier()
    for tag, idir in (("A", root / "index_single"), ("B", root / "index_parts")):
        s = SearchIndexFactory("video", FID, {"features_dir": root / "features", "index_dir": idir})
        assert s.load_index(ITYPE) is True
        idx = s.index
        assert type(idx) is ShardedFlatIPIndex and type(idx.local) is _CpuFlatL2 and idx.ntotal == N
        if tag == "A":
            lo, hi = shard_range(N, rank, world)
            assert idx.local.ntotal == hi - lo and idx.local.reserved == hi - lo
        with pytest.raises(NotImplementedError) as e:
            idx.search(Q, 3, params=SearchParameters(sel=IDSelectorRange(0, 10)))
        assert str(e.value) == NO_SELECTOR
        with pytest.raises(NotImplementedError):
            idx.range_search(Q, 0.1)
        with pytest.raises(NotImplementedError):
            idx.remove_ids(np.array([1]))
        with pytest.raises(NotImplementedError):
            s.update_index(ITYPE)
        out[f"{tag}_local"] = np.array([idx.local.ntotal])
        out[f"{tag}_local_ids"] = idx.local.ids
        out[f"{tag}_dist"], out[f"{tag}_ids"] = s.search("video", "dog", topk=7)
        out[f"{tag}_D"], out[f"{tag}_I"] = idx.search(Q, 25)
        out[f"{tag}_Dpad"], out[f"{tag}_Ipad"] = idx.search(Q[:1], N + 5)     # more than the index holds: padded behind the merge
        out[f"{tag}_rec"] = idx.reconstruct_batch(np.array(WANT_IDS, dtype=np.int64))
    np.savez(root / f"flatl2_rank{rank}.npz", **out)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_through_the_plugin_surface_world2(tmp_path):
    from wise_amd.index.search_index_factory import SearchIndexFactory
    from wise_amd.index.sharded import shard_range

    N, d, world = 1001, 32, 2
    X = rows_of_mixed_length(N, d, 5)
    X[700] = X[20]                                                       # equal rows on both ranks' slices
    ids = np.arange(N, dtype=np.int64) + 1
    _write_store(tmp_path / "features", X, ids, per_file=100)           # 11 tar files: ranks get 6 and 5 of them
    single = SearchIndexFactory("video", FID, {"features_dir": tmp_path / "features", "index_dir": tmp_path / "index_single"})
    single.create_index(ITYPE)                                           # no process group here: the one-file build, no GPU needed
    assert faiss_io.read_idmap_flat_l2(single.get_index_filename(ITYPE))[0].tobytes() == X.tobytes()
    mp.spawn(_plugin_worker, args=(world, _free_port(), str(tmp_path), N, d), nprocs=world, join=True)

    q = _FakeTextTower(d).extract_text_features(["This is a photo of a dog"])
    Q = rows_of_mixed_length(3, d, 6)
    D1, I1 = ref.topk(X, q, 7, ids=ids)
    D3, I3 = ref.topk(X, Q, 25, ids=ids)
    Dp, Ip = ref.topk(X, Q[:1], N + 5, ids=ids)
    rec_ref = np.full((4, d), np.nan, np.float32)
    for i, w in enumerate(WANT_IDS):
        if w <= N:
            rec_ref[i] = X[w - 1]
    locals_ = []
    for r in range(world):
        g = np.load(tmp_path / f"flatl2_rank{r}.npz")
        lo, hi = shard_range(N, r, world)
        assert np.array_equal(g["A_local_ids"], ids[lo:hi])
        for tag in "AB":
            assert np.array_equal(g[f"{tag}_ids"], I1[0]) and np.array_equal(g[f"{tag}_dist"], D1[0]), (r, tag)
            assert np.array_equal(g[f"{tag}_rec"], rec_ref, equal_nan=True), (r, tag)
            assert np.array_equal(g[f"{tag}_Dpad"], Dp) and (g[f"{tag}_Ipad"][0, N:] == -1).all(), (r, tag)   # +3.4028235e38 behind the rows
        # (A) slices of the one file in its order: the answer is the one-process answer, bits and ids
        assert np.array_equal(g["A_I"], I3) and np.array_equal(g["A_D"], D3) and np.array_equal(g["A_Ipad"], Ip), r
        locals_.append(int(g["B_local"][0]))
    assert locals_ == [501, 500]                                         # tar files 0,2,..,10 (5 x 100 + the 1-row tail) and 1,3,..,9
    # (B) the parts are the store's shards dealt round-robin: the same rows in another order — the same distances, and the same ids
    # wherever the distances differ
    for r in range(world):
        g = np.load(tmp_path / f"flatl2_rank{r}.npz")
        assert np.array_equal(g["B_D"], D3), r
        assert all(set(a.tolist()) == set(b.tolist()) for a, b in zip(g["B_I"], I3)), r

"""CPU tests (-m "not gpu") of IndexSQfp16L2: the entry points are declared, exported and bound; the index file ('IxMp' around 'IxSQ',
qtype 4, metric_type 1) and what each of the two binary16 readers does with the other's file; the type's name in the plugin; the plugin
surface over a numpy stand-in for FlatSQfp16L2Index; the restatement against float64; the two recorded studies.  The kernels
themselves: tests/test_gpu_sqfp16_l2.py."""
import hashlib
import json
import re
import struct
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import l2_flat_ref  # noqa: E402
import sqfp16_l2_ref as ref  # noqa: E402
from wise_amd import _lib  # noqa: E402
from wise_amd.index import faiss_io  # noqa: E402

ITYPE = "IndexSQfp16L2"
FID = "mlfoundations/open_clip/ViT-B-32/seeded-0"
GOLDEN = ROOT / "tests" / "golden"
# entry point -> number of arguments
NEW_SYMBOLS = {"wise_l2sq16_topk": 13, "wise_l2sq16_topk_pos": 15, "wise_l2sq16_range_count": 11, "wise_l2sq16_range_fill": 14,
               "wise_l2sq16_prepare": 6, "wise_l2sq16_topk_batched": 16}
NEW_SIZES = {"wise_l2sqfp16_topk_workspace_bytes": 4, "wise_l2sqfp16_range_workspace_bytes": 3, "wise_l2sqfp16_topk_batched_workspace_bytes": 4}


def rows_of_mixed_length(n, d, seed):
    """rows that are NOT normalised: lengths spread over 1 .. 4, where L2 and the inner product rank differently"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, d)) / np.sqrt(d) * rng.uniform(1.0, 4.0, size=(n, 1))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
def test_entry_points_declared_exported_and_bound():
    from wise_amd.build import HIP_SOURCES, CSRC, declared_symbols

    declared = set(declared_symbols())
    assert set(_lib.SIGNATURES) == declared
    assert "l2_sq16.hip" in HIP_SOURCES and (CSRC / "l2_sq16.hip").exists() and "struct Codec16L2" in (CSRC / "sq_codec.h").read_text()
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
    assert "wise_l2sq16_" in header.split("int wise_abi_version(void);")[0]          # listed as added within 5
    assert header.count("THE DISTANCE IS A CONTRACT") == 2 and "THE DISTANCE IS A CONTRACT" in ref.__doc__
    integration = (ROOT / "INTEGRATION.md").read_text()
    for name in list(NEW_SYMBOLS) + list(NEW_SIZES):
        assert name in integration, name


def test_workspace_functions_answer_without_a_device():
    lib = _lib.load()
    assert lib.wise_l2sqfp16_topk_workspace_bytes(1000, 64, 4, 10) > 0
    assert lib.wise_l2sqfp16_topk_workspace_bytes(0, 64, 1, 10) > 0                   # an empty index is searched: all padding
    assert lib.wise_l2sqfp16_topk_workspace_bytes(70001, 16, 1024, 2048) > 0 and lib.wise_l2sqfp16_topk_workspace_bytes(1000, 1024, 1, 1) > 0
    for N, d, nq, k in ((1000, 20, 1, 10), (1000, 8, 1, 10), (1000, 1040, 1, 10), (1000, 64, 0, 10), (1000, 64, 1025, 10),
                        (1000, 64, 1, 0), (1000, 64, 1, 2049), (-1, 64, 1, 10), ((1 << 32) - 1, 64, 1, 10)):
        assert lib.wise_l2sqfp16_topk_workspace_bytes(N, d, nq, k) == 0, (N, d, nq, k)
    assert lib.wise_l2sqfp16_range_workspace_bytes(5000, 64, 3) > 0 and lib.wise_l2sqfp16_range_workspace_bytes(0, 64, 3) >= 0
    for N, d, nq in ((5000, 20, 3), (5000, 64, 0), (5000, 64, 65536), (-1, 64, 3)):
        assert lib.wise_l2sqfp16_range_workspace_bytes(N, d, nq) == 0, (N, d, nq)
    # the batched search is served where its siblings are, and takes their workspace plus one more array of per-query floats (|q|^2)
    for d in (256, 512, 768, 1024):
        assert lib.wise_l2sqfp16_topk_batched_workspace_bytes(4096, d, 3, 128) > 0
        assert lib.wise_l2sqfp16_topk_batched_workspace_bytes(40000, d, 130, 10) == lib.wise_l2_topk_batched_workspace_bytes(40000, d, 130, 10)
    for N, d, nq, k in ((4095, 512, 64, 10), (40000, 512, 2, 10), (40000, 512, 64, 129), (40000, 128, 64, 10), (40000, 320, 64, 10),
                        (40000, 20, 64, 10), (1 << 31, 512, 64, 10), (40000, 512, 1025, 10)):
        assert lib.wise_l2sqfp16_topk_batched_workspace_bytes(N, d, nq, k) == 0, (N, d, nq, k)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
@pytest.mark.parametrize("d", [16, 48, 512, 1024])
def test_restatement_equals_the_float64_distance_within_its_rounding_term(d):
    X, Q = rows_of_mixed_length(300, d, d), rows_of_mixed_length(4, d, d + 1)
    X[7] *= np.float32(2.0 ** -16)                                       # a row of binary16 subnormals
    H = ref.encode(X)
    H[5] = ref.encode(Q[:1])[0]
    Q[0] = H[5].astype(np.float32)                                       # a distance of exactly +0
    Q[1] = H[6].astype(np.float32) * np.float32(1.0 + 2.0 ** -20)        # heavy cancellation in every difference
    mag = np.abs(H[7].astype(np.float32))
    assert ((mag > 0) & (mag < 2.0 ** -14)).any()
    S = ref.dists(H, Q)
    assert S.dtype == np.float32 and S[0, 5] == 0 and not np.signbit(S[0, 5]) and (S >= 0).all()
    err = np.abs(S.astype(np.float64) - ref.real_dists(H, Q))
    term = ref.rounding_term(d, Q, H)
    assert (err <= term[:, None]).all(), (err.max(), term.min())
    # the chain's order is the contract's: element i of chunk c is e = 8 c + i (i < 8), d / 2 + 8 c + i - 8 (i >= 8) — Codec16's
    C = d // 16
    e = np.array([[8 * c + i if i < 8 else d // 2 + 8 * c + i - 8 for i in range(16)] for c in range(C)])
    assert np.array_equal(ref.chunked(np.arange(d, dtype=np.float32)[None])[0], e.astype(np.float32))
    # on rows that are exactly representable the distance is IndexFlatL2's up to the order of the sum: both within the rounding term
    S32 = l2_flat_ref.dists(H.astype(np.float32), Q)
    assert (np.abs(S.astype(np.float64) - S32.astype(np.float64)) <= 2 * term[:, None]).all()
    # selection: ascending distance, ties to the lower position, faiss's L2 padding
    H[200] = H[100]
    D, I = ref.topk(H, H[100:101].astype(np.float32), 5)
    assert I[0, :2].tolist() == [100, 200] and D[0, 0] == D[0, 1] == 0 and (np.diff(D[0]) >= 0).all()
    D, I = ref.topk(H[:3], Q, 5, id_base=7)
    assert (I[:, 3:] == -1).all() and (D[:, 3:] == np.float32(3.4028235e38)).all() and (I[:, :3] >= 7).all()
    S = ref.dists(H, Q)
    radius = float(np.sort(S, axis=1)[:, 10].max())
    lims, Dr, Ir = ref.range_search(H, Q, radius, S=S)
    for q in range(4):
        seg = Dr[lims[q]:lims[q + 1]]
        assert len(seg) >= 10 and (np.diff(seg) >= 0).all() and (seg < np.float32(radius)).all()
    # the half-norms: the fixed order against float64, and the largest norm
    half = ref.half_norms(H)
    real = 0.5 * (H.astype(np.float64) ** 2).sum(axis=1)
    assert half.dtype == np.float32 and (np.abs(half.astype(np.float64) - real) <= d * 2.0 ** -24 * real + 1e-45).all()
    assert ref.max_norm(half).dtype == np.float32 and abs(float(ref.max_norm(half)) - np.sqrt(2 * real.max())) <= 1e-6 * np.sqrt(2 * real.max())
    assert float(ref.max_norm(np.zeros(0, np.float32))) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the studies
def test_recorded_quality_study():
    """What the rows' rounding to binary16 costs under L2 on the study set of the inverted-file L2 type: seed 0 is recomputed, the
    other four seeds are read from the record."""
    import ivf_l2_ref

    gold = json.loads((GOLDEN / "sqfp16_l2_quality.json").read_text())
    assert json.dumps(ivf_l2_ref.STUDY) in gold["what"] and gold["seeds"] == [0, 1, 2, 3, 4] and len(gold["runs"]) == 5
    run = ref.quality_study(0)
    rec = gold["runs"][0]
    assert set(run) == set(rec)
    for key, v in run.items():
        assert v == pytest.approx(rec[key], rel=1e-6), key
    for r in gold["runs"]:
        assert 0.0 < r["max_abs_dist_gap"] <= r["bound"] and 0.0 < r["gap_over_bound_max"] < 1.0
        assert r["recall"] >= 0.99 and r["recall_flat_l2"] >= r["recall"]           # near-lossless: the IP twin's finding
    assert gold["recall_min"] == min(r["recall"] for r in gold["runs"])
    assert gold["max_abs_dist_gap"] == max(r["max_abs_dist_gap"] for r in gold["runs"])


def test_recorded_error_band_of_the_batched_search():
    """eps of wise_l2sq16_topk_batched, term by term: observed <= bound for every term and for their sum, every row of the exact top-k
    is listed, and the longest list is far from the 4096 rows a list holds.  d = 256 is recomputed here; d = 1024 is read from the
    record (python tests/sqfp16_l2_ref.py rewrites both records)."""
    gold = json.loads((GOLDEN / "sqfp16_l2_band.json").read_text())
    assert json.dumps(ref.STUDY) in gold["what"] and [r["d"] for r in gold["runs"]] == [256, 1024]
    assert ref.STUDY["rows"] == 40000 and ref.STUDY["queries"] == 64 and ref.STUDY["k"] == 10
    run = ref.band_study(256)
    assert set(run["terms"]) == {"query_rounding", "accumulation", "half_norm", "contract"}       # no row-rounding term
    rec = gold["runs"][0]
    assert run["seed"] == rec["seed"] == 0 and run["longest_list"] == rec["longest_list"] and run["topk_rows_listed"] is True
    for name, t in list(run["terms"].items()) + [("total", run["total"])]:
        g = rec["terms"][name] if name != "total" else rec["total"]
        assert t["observed"] == pytest.approx(g["observed"], rel=1e-6) and t["bound"] == pytest.approx(g["bound"], rel=1e-9), name
    for r in gold["runs"] + [run]:
        for name, t in list(r["terms"].items()) + [("total", r["total"])]:
            assert 0.0 < t["observed"] <= t["bound"] and t["ratio"] < 1.0, (r["d"], name, t)
        assert r["topk_rows_listed"] is True and r["longest_list"] < 4096, r["longest_list"]
        assert abs(r["max_row_norm_prepare"] - r["max_row_norm"]) <= 1e-6 * r["max_row_norm"]
        # the band's own M is 1.001 norms[0]: the prepared norm never undercuts the real one by more than that
        assert r["max_row_norm_prepare"] * 1.001 >= r["max_row_norm"]


# ---------------------------------------------------------------------------------------------------------------------
# the file
@pytest.mark.parametrize("n", [0, 1, 77])
def test_file_round_trip_is_byte_stable(tmp_path, n):
    d = 32
    H, ids = ref.encode(rows_of_mixed_length(n, d, 3)), (np.arange(n, dtype=np.int64) * 7 + 5)
    fn = tmp_path / "a.faiss"
    faiss_io.write_idmap_sq16_l2(fn, H, ids)
    raw = fn.read_bytes()
    # the layout, restated: 'IxMp' + header, 'IxSQ' + header, both with metric_type 1, the ScalarQuantizer record with qtype 4, codes, id map
    hdr = struct.pack("<iqqq?i", d, n, 1 << 20, 1 << 20, True, 1)
    want = (b"IxMp" + hdr + b"IxSQ" + hdr + struct.pack("<iifQQ", 4, 0, 0.0, d, 2 * d) + struct.pack("<Q", 0)
            + struct.pack("<Q", n * 2 * d) + H.astype("<f2").tobytes() + struct.pack("<Q", n) + ids.tobytes())
    assert raw == want
    digests = json.loads((GOLDEN / "sqfp16_l2_file_digests.json").read_text())
    assert hashlib.sha256(raw).hexdigest() == digests[f"n={n}"]
    assert faiss_io.index_fourcc(fn) == "IxMp" and faiss_io.index_fourcc(fn, inner=True) == "IxSQ"
    assert faiss_io.flat_sq_qtype(fn) == 4 and faiss_io.flat_sq_metric(fn) == 1
    assert faiss_io.idmap_sq16_l2_ntotal(fn) == faiss_io.index_ntotal(fn) == n
    for mmap in (True, False):
        H2, ids2 = faiss_io.read_idmap_sq16_l2(fn, mmap=mmap)
        assert H2.dtype == np.float16 and H2.shape == (n, d) and H2.tobytes() == H.tobytes() and np.array_equal(ids2, ids)
        assert isinstance(H2, np.memmap) == (mmap and n > 0)
    st = faiss_io.read_index(fn)
    assert set(st) == {"halves", "ids", "metric"} and st["metric"] == "l2" and st["halves"].tobytes() == H.tobytes()
    again = tmp_path / "b.faiss"
    faiss_io.write_index(again, st)
    assert again.read_bytes() == raw
    for lo, hi in ((0, n), (n // 3, n - n // 4), (n, n)):
        Hr, idr = faiss_io.read_idmap_sq16_l2_range(fn, lo, hi)
        assert Hr.tobytes() == H[lo:hi].tobytes() and np.array_equal(idr, ids[lo:hi])
        rr = faiss_io.read_index_range(fn, lo, hi)
        assert rr["halves"].tobytes() == H[lo:hi].tobytes() and np.array_equal(rr["ids"], ids[lo:hi]) and rr["metric"] == "l2"
    with pytest.raises(ValueError, match="outside"):
        faiss_io.read_idmap_sq16_l2_range(fn, 0, n + 1)
    # the inner-product file of the same rows differs in its two metric fields only
    ip = tmp_path / "ip.faiss"
    faiss_io.write_idmap_sq16_ip(ip, H, ids)
    a = ip.read_bytes()
    assert len(a) == len(raw) and [i for i in range(len(a)) if a[i] != raw[i]] == [4 + 29, 4 + 33 + 4 + 29]
    assert faiss_io.flat_sq_metric(ip) == 0 and set(faiss_io.read_index(ip)) == {"halves", "ids"}


def test_each_binary16_reader_refuses_the_other_metric_by_name(tmp_path):
    n, d = 6, 16
    H, ids = ref.encode(rows_of_mixed_length(n, d, 5)), np.arange(n, dtype=np.int64)
    l2, ip = tmp_path / "l2.faiss", tmp_path / "ip.faiss"
    faiss_io.write_idmap_sq16_l2(l2, H, ids)
    faiss_io.write_idmap_sq16_ip(ip, H, ids)
    # the L2 reader refuses a metric-0 file by name; the inner-product reader a metric-1 file; each still reads its own
    for call in (faiss_io.read_idmap_sq16_l2, faiss_io.idmap_sq16_l2_ntotal, lambda p: faiss_io.read_idmap_sq16_l2_range(p, 0, 1)):
        with pytest.raises(RuntimeError, match=re.escape(str(ip))) as e:
            call(ip)
        assert "IndexSQfp16L2" in str(e.value) and "metric_type 0" in str(e.value)
    for call in (faiss_io.read_idmap_sq16_ip, faiss_io.idmap_sq16_ip_ntotal, lambda p: faiss_io.read_idmap_sq16_ip_range(p, 0, 1)):
        with pytest.raises(RuntimeError, match=re.escape(str(l2))) as e:
            call(l2)
        assert "IndexSQfp16 " in str(e.value) and "metric_type 1" in str(e.value)
    assert faiss_io.read_idmap_sq16_ip(ip)[0].tobytes() == faiss_io.read_idmap_sq16_l2(l2)[0].tobytes() == H.tobytes()
    # one header alone with the other metric is refused too
    raw = l2.read_bytes()
    inner_metric, outer_metric = 4 + 33 + 4 + 29, 4 + 29
    for what, at in (("inner", inner_metric), ("outer", outer_metric)):
        fn = tmp_path / f"l2_metric0_{what}.faiss"
        fn.write_bytes(raw[:at] + struct.pack("<i", 0) + raw[at + 4:])
        with pytest.raises(RuntimeError, match=re.escape(str(fn))) as e:
            faiss_io.read_idmap_sq16_l2(fn)
        assert "IndexSQfp16L2" in str(e.value) and "metric_type" in str(e.value)
    # a bare 'IxSQ' record with metric_type 1 reads with ids equal to positions
    bare = tmp_path / "bare.faiss"
    bare.write_bytes(raw[4 + 33:len(raw) - 8 - 8 * n])
    Hb, idb = faiss_io.read_idmap_sq16_l2(bare)
    assert Hb.tobytes() == H.tobytes() and np.array_equal(idb, np.arange(n)) and faiss_io.flat_sq_metric(bare) == 1
    # cut files, the 8-bit file and the fp32 files are refused by name
    for cut in (2, 8 * n, 8 * n + 8 + 5, len(raw) - 50, len(raw) - 10):
        fn = tmp_path / f"short_{cut}.faiss"
        fn.write_bytes(raw[:len(raw) - cut])
        with pytest.raises(RuntimeError, match=re.escape(str(fn))):
            faiss_io.read_idmap_sq16_l2(fn)
    sq8 = tmp_path / "sq8.faiss"
    faiss_io.write_idmap_sq8_ip(sq8, np.ones(2 * d, np.float32), np.zeros((n, d), np.uint8), ids)
    flat = tmp_path / "flat.faiss"
    faiss_io.write_idmap_flat_l2(flat, H.astype(np.float32), ids)
    for other in (sq8, flat):
        with pytest.raises(RuntimeError, match=re.escape(str(other))):
            faiss_io.read_idmap_sq16_l2(other)
    assert faiss_io.flat_sq_metric(flat) is None
    with pytest.raises(RuntimeError, match="No such file"):
        faiss_io.read_idmap_sq16_l2(tmp_path / "missing.faiss")


# ---------------------------------------------------------------------------------------------------------------------
# a numpy stand-in for FlatSQfp16L2Index: what FeatureSearchIndex.flat_sqfp16_l2_index_factory must offer
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


class _CpuFlatSQL2:
    """reserve / add_with_ids / add_halves_with_ids / search_device / search / range_search / remove_ids / reconstruct_batch /
    _selector_rows / rows_host and `metric`: every answer by tests/sqfp16_l2_ref.py."""
    metric = "l2"

    def __init__(self, d):
        self.d, self.device = int(d), torch.device("cpu")
        self.H, self.ids = np.zeros((0, d), np.float16), np.zeros(0, np.int64)
        self.is_trained = True

    def reserve(self, n):
        self.reserved = int(n)

    def add_with_ids(self, x, ids):
        self.add_halves_with_ids(ref.encode(np.asarray(x, np.float32)), ids)

    def add_halves_with_ids(self, h, ids):
        assert np.asarray(h).dtype == np.float16
        self.H = np.concatenate([self.H, np.asarray(h)])
        self.ids = np.concatenate([self.ids, np.asarray(ids, np.int64)])

    @property
    def ntotal(self):
        return self.H.shape[0]

    def _selector_rows(self):
        return torch.from_numpy(self.ids), 0, self.ntotal

    def rows_host(self):
        return self.H, self.ids

    def search_device(self, q, k, sel=None):
        Q = q.numpy()
        pos = np.arange(self.ntotal) if sel is None else np.flatnonzero(_selected(sel, self.ids))
        D, I = ref.topk_pos(self.H, Q, k, pos, ids=self.ids)
        return torch.from_numpy(D), torch.from_numpy(I)

    def search(self, x, k, params=None):
        D, I = self.search_device(torch.from_numpy(np.ascontiguousarray(x, np.float32)), k, None if params is None else params.sel)
        return D.numpy(), I.numpy()

    def range_search(self, x, thresh, params=None):
        keep = None if params is None or params.sel is None else _selected(params.sel, self.ids)
        return ref.range_search(self.H, np.ascontiguousarray(x, np.float32), thresh, ids=self.ids, keep=keep)

    def remove_ids(self, sel):
        from wise_amd.index.selector import as_selector
        gone = _selected(as_selector(sel), self.ids)
        self.H, self.ids = self.H[~gone], self.ids[~gone]
        return int(gone.sum())

    def reconstruct_batch(self, want):
        out = np.full((len(want), self.d), np.nan, np.float32)
        for i, w in enumerate(want):
            hit = np.flatnonzero(self.ids == w)
            if len(hit):
                out[i] = self.H[hit[0]].astype(np.float32)
        return out


class _FakeTextTower:
    def __init__(self, d):
        self.d = d

    def extract_text_features(self, texts):
        import zlib
        out = np.stack([np.random.default_rng(zlib.crc32(t.encode())).standard_normal(self.d) for t in texts])
        return (2.0 * out / np.sqrt(self.d)).astype(np.float32)


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
def test_type_name_is_in_the_plugin_table_and_the_pinned_names_stay(tmp_path, monkeypatch):
    from wise_amd.index import feature_search_index as fsi
    from wise_amd.index import sharded
    from wise_amd.index.flat_common import FlatIndexBase
    from wise_amd.index.flat_sq import FlatSQfp16IPIndex, FlatSQfp16L2Index
    from wise_amd.index.selector import IDSelectorRange

    row = fsi.FLAT_TYPES[ITYPE]
    assert fsi._family(ITYPE) is None and fsi.parse_pq_flat_type(ITYPE) is None
    assert row.fourcc == "IxSQ" and row.qtype == faiss_io.QT_FP16 == 4 and row.metric == "l2" and row.dtype is np.float16
    assert row.trained is False and row.add == "add_halves_with_ids" and row.factory == "flat_sqfp16_l2_index_factory"
    assert row.writer is faiss_io.write_idmap_sq16_l2 and row.reader is faiss_io.read_idmap_sq16_l2
    assert row.encode is fsi.FLAT_TYPES["IndexSQfp16"].encode and fsi.FLAT_TYPES["IndexSQfp16"].metric == "ip"
    assert [t for t, f in fsi.FLAT_TYPES.items() if f.trained] == ["IndexSQ8bit"]      # the new type is untrained
    assert fsi.FeatureSearchIndex.flat_sqfp16_l2_index_factory is FlatSQfp16L2Index and issubclass(FlatSQfp16L2Index, FlatIndexBase)
    assert FlatSQfp16L2Index.metric == "l2" and FlatSQfp16IPIndex.metric == "ip"
    assert FlatSQfp16L2Index.BATCH_MIN_ROWS == 1 << 18 and FlatSQfp16L2Index.BATCH_MIN_QUERIES >= 3
    assert "IndexSQfp16L2" in fsi.__doc__ and "FlatSQfp16L2Index" in fsi.__doc__
    for name in ("IndexSQ8bitL2", "IndexIVFSQ8L2", "IndexSQfp16L2 ", "IndexSQfp16l2", "IndexIVFSQfp16L2"):   # none of these is built
        assert name not in fsi.FLAT_TYPES and fsi._family(name) is None
    si = _factory(tmp_path)
    assert si.get_index_filename(ITYPE).name == "video-IndexSQfp16L2.faiss"
    with pytest.raises(NotImplementedError, match="IndexSQfp16, and IndexFlatL2$"):    # the unknown-type text is as it was
        si.create_index("IndexSQ8bitL2")
    _write_store(tmp_path / "features", rows_of_mixed_length(12, 64, 9), np.arange(12) + 1)
    with pytest.raises(FileNotFoundError, match="create_index"):
        si.update_index(ITYPE)
    # the shape check fires before the store is read
    _write_store(tmp_path / "b" / "features", rows_of_mixed_length(12, 40, 9), np.arange(12) + 1)
    monkeypatch.setattr(fsi, "_read_store", lambda store: pytest.fail("the store was read before the shape check"))
    with pytest.raises(ValueError, match="IndexSQfp16L2.*multiple of 16"):
        _factory(tmp_path / "b").create_index(ITYPE)
    with pytest.raises(ValueError, match="IndexSQfp16L2.*multiple of 16"):
        FlatSQfp16L2Index(40, device="cpu")
    with pytest.raises(ValueError, match="multiple of 16"):
        FlatSQfp16L2Index(1040, device="cpu")
    sh = sharded.ShardedFlatIPIndex(FlatSQfp16L2Index(32, device="cpu"))  # the sharded wrapper keeps its three refusals
    with pytest.raises(NotImplementedError, match="no selector"):
        sh.search_device(None, 5, sel=IDSelectorRange(0, 10))
    with pytest.raises(NotImplementedError, match="collective removal is not built"):
        sh.remove_ids(np.array([1]))
    with pytest.raises(NotImplementedError):
        sh.range_search(np.zeros((1, 32), np.float32), 0.1)


# ---------------------------------------------------------------------------------------------------------------------
# the plugin in one process
def test_plugin_create_load_search_update_with_a_stand_in(tmp_path, monkeypatch):
    from wise_amd.index import feature_search_index as fsi
    from wise_amd.index.selector import IDSelectorRange

    N, d = 300, 32
    X, ids = rows_of_mixed_length(N, d, 11), np.arange(N, dtype=np.int64) * 2 + 1
    X[200] = X[10]                                                       # equal rows: the lower position wins
    H = ref.encode(X)
    _write_store(tmp_path / "features", X, ids, per_file=64)
    monkeypatch.setattr(fsi.FeatureSearchIndex, "flat_sqfp16_l2_index_factory", _CpuFlatSQL2)
    monkeypatch.setattr(fsi, "FeatureExtractorFactory", lambda fid: _FakeTextTower(d))
    si = _factory(tmp_path)
    si.create_index(ITYPE)
    fn = si.get_index_filename(ITYPE)
    assert faiss_io.index_fourcc(fn, inner=True) == "IxSQ" and faiss_io.flat_sq_metric(fn) == 1 and faiss_io.flat_sq_qtype(fn) == 4
    Hf, idf = faiss_io.read_idmap_sq16_l2(fn)
    assert Hf.tobytes() == H.tobytes() and np.array_equal(idf, ids)      # the rows rounded to binary16 on the host: the encoder's bits
    before = fn.read_bytes()
    si.create_index(ITYPE)                                               # skip-if-exists
    assert fn.read_bytes() == before
    assert si.load_index(ITYPE) is True                                  # the record's metric_type decides between the two qtype-4 files
    assert type(si.index) is _CpuFlatSQL2 and si.index.ntotal == N and si.index.reserved == N and si.index.H.tobytes() == H.tobytes()

    tower = _FakeTextTower(d)
    q = tower.extract_text_features(["This is a photo of a dog"])
    D1, I1 = ref.topk(H, q, 7, ids=ids)
    dist_, ids_ = si.search("video", "dog", topk=7)
    assert np.array_equal(ids_, I1[0]) and np.array_equal(dist_, D1[0]) and (np.diff(dist_) >= 0).all()
    ip_order = ids[np.argsort(-(X.astype(np.float64) @ q[0].astype(np.float64)), kind="stable")[:7]]
    assert not np.array_equal(ip_order, I1[0])                           # on these rows the inner product ranks differently
    words = ["dog", "cat", "a red car", "rain"]
    Qb = tower.extract_text_features(["This is a photo of a " + w for w in words])
    Db, Ib = ref.topk(H, Qb, 5, ids=ids)
    got = si.search_batch("video", words, topk=5)
    assert len(got) == 4 and all(np.array_equal(g[0], Db[i]) and np.array_equal(g[1], Ib[i]) for i, g in enumerate(got))
    chosen = ids[5:60:3]                                                 # within: an array of ids and a selector
    Dw, Iw = ref.topk_pos(H, q, 7, np.flatnonzero(np.isin(ids, chosen)), ids=ids)
    dw, iw = si.search("video", "dog", topk=7, within=chosen)
    assert np.array_equal(iw, Iw[0]) and np.array_equal(dw, Dw[0]) and set(iw.tolist()) <= set(chosen.tolist())
    gw = si.search_batch("video", words, topk=5, within=IDSelectorRange(101, 301))
    in_range = np.flatnonzero((ids >= 101) & (ids < 301))
    Dr, Ir = ref.topk_pos(H, Qb, 5, in_range, ids=ids)
    assert all(np.array_equal(g[0], Dr[i]) and np.array_equal(g[1], Ir[i]) for i, g in enumerate(gw))
    radius = float(np.sort(ref.dists(H, q)[0])[19])                      # search_range: every row below the radius, ascending
    lims, Dg, Ig = ref.range_search(H, q, radius, ids=ids)
    assert lims[1] == 19
    dr, ir = si.search_range("video", "dog", radius)
    assert np.array_equal(dr, Dg) and np.array_equal(ir, Ig) and (np.diff(dr) >= 0).all()

    # update_index: 40 vectors leave the store, 25 new ones arrive; the file stays an 'IxSQ' file of metric_type 1
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
    assert faiss_io.index_fourcc(fn, inner=True) == "IxSQ" and faiss_io.flat_sq_metric(fn) == 1
    H2, id2 = faiss_io.read_idmap_sq16_l2(fn)
    added = sid[np.isin(sid, new_ids)]                                   # in store order, behind the kept rows in their order
    assert np.array_equal(id2, np.concatenate([ids[stay], added]))
    assert H2.tobytes() == np.concatenate([H[stay], ref.encode(sX[np.isin(sid, new_ids)])]).tobytes()
    assert si.update_index(ITYPE) == (0, 0)
    assert si.load_index(ITYPE) is True and si.index.ntotal == N - 40 + 25
    D3, I3 = ref.topk(np.asarray(H2), q, 7, ids=id2)
    dist3, ids3 = si.search("video", "dog", topk=7)
    assert np.array_equal(ids3, I3[0]) and np.array_equal(dist3, D3[0])
    # and IndexSQfp16 beside it, same store and same payload dtype: its file stays metric_type 0 through an update and loads as itself

    class _CpuFlatSQIP(_CpuFlatSQL2):
        metric = "ip"
    monkeypatch.setattr(fsi.FeatureSearchIndex, "flat_sqfp16_index_factory", _CpuFlatSQIP)
    si.create_index("IndexSQfp16")
    fip = si.get_index_filename("IndexSQfp16")
    assert faiss_io.flat_sq_metric(fip) == 0 and faiss_io.read_idmap_sq16_ip(fip)[0].tobytes() == ref.encode(sX).tobytes()
    shutil.rmtree(tmp_path / "features")
    _write_store(tmp_path / "features", sX[:-3], sid[:-3], per_file=64)
    assert si.update_index("IndexSQfp16") == (0, 3) and faiss_io.flat_sq_metric(fip) == 0
    assert si.load_index("IndexSQfp16") is True and type(si.index) is _CpuFlatSQIP
    assert si.load_index(ITYPE) is True and type(si.index) is _CpuFlatSQL2

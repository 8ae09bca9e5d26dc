"""CPU tests (-m "not gpu") of IndexSQfp16: the entry points are declared, exported and bound; the index file ('IxMp' around 'IxSQ');
the type's name in the plugin; the plugin surface over a numpy stand-in for FlatSQfp16IPIndex, in one process and at world size 2
(gloo); and the recorded quality study.  The kernels themselves: tests/test_gpu_sqfp16_flat.py."""
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

import sqfp16_flat_ref as ref  # noqa: E402
from wise_amd import _lib  # noqa: E402
from wise_amd.index import faiss_io  # noqa: E402

ITYPE = "IndexSQfp16"
FID = "mlfoundations/open_clip/ViT-B-32/seeded-0"
# entry point -> number of arguments
NEW_SYMBOLS = {"wise_ipsq16_topk": 13, "wise_ipsq16_topk_pos": 15, "wise_ipsq16_range_count": 11, "wise_ipsq16_range_fill": 14,
               "wise_ipsq16_reconstruct": 9, "wise_ipsq16_prepare": 5, "wise_ipsq16_topk_batched": 15}
NEW_SIZES = {"wise_ipsqfp16_topk_workspace_bytes": 4, "wise_ipsqfp16_range_workspace_bytes": 3, "wise_ipsqfp16_topk_batched_workspace_bytes": 4}


def unit_rows(n, d, seed):
    X = np.random.default_rng(seed).standard_normal((n, d))
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
def test_entry_points_declared_exported_and_bound():
    from wise_amd.build import HIP_SOURCES, CSRC, declared_symbols

    declared = set(declared_symbols())
    assert set(_lib.SIGNATURES) == declared
    assert "ip_sq16.hip" in HIP_SOURCES and (CSRC / "ip_sq16.hip").exists() and (CSRC / "sq_codec.h").exists()
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
    assert "wise_ipsq16_" in header.split("int wise_abi_version(void);")[0]          # listed as added within 5
    integration = (ROOT / "INTEGRATION.md").read_text()
    for name in list(NEW_SYMBOLS) + list(NEW_SIZES):
        assert name in integration, name


def test_workspace_functions_answer_without_a_device():
    lib = _lib.load()
    assert lib.wise_ipsqfp16_topk_workspace_bytes(1000, 64, 4, 10) > 0
    assert lib.wise_ipsqfp16_topk_workspace_bytes(0, 64, 1, 10) > 0                 # an empty index is searched: all padding
    for N, d, nq, k in ((1000, 20, 1, 10), (1000, 8, 1, 10), (1000, 1040, 1, 10), (1000, 64, 0, 10), (1000, 64, 1025, 10),
                        (1000, 64, 1, 0), (1000, 64, 1, 2049), (-1, 64, 1, 10)):
        assert lib.wise_ipsqfp16_topk_workspace_bytes(N, d, nq, k) == 0, (N, d, nq, k)
    assert lib.wise_ipsqfp16_range_workspace_bytes(5000, 64, 3) > 0 and lib.wise_ipsqfp16_range_workspace_bytes(5000, 20, 3) == 0
    # the batched search: d % 128 == 0 in [256, 1024], nq >= 3, k <= 128, N >= 4096 — and NO large-N floor beyond that
    for d in (256, 512, 768, 1024):
        assert lib.wise_ipsqfp16_topk_batched_workspace_bytes(4096, d, 3, 128) > 0
        assert lib.wise_ipsqfp16_topk_batched_workspace_bytes(40000, d, 130, 10) > 0
    for N, d, nq, k in ((4095, 512, 64, 10), (40000, 512, 2, 10), (40000, 512, 64, 129), (40000, 128, 64, 10), (40000, 320, 64, 10),
                        (40000, 20, 64, 10), (1 << 31, 512, 64, 10)):
        assert lib.wise_ipsqfp16_topk_batched_workspace_bytes(N, d, nq, k) == 0, (N, d, nq, k)


# ---------------------------------------------------------------------------------------------------------------------
# the file
def _halves(n, d, seed):
    return ref.encode(unit_rows(n, d, seed))


@pytest.mark.parametrize("n", [0, 1, 77])
def test_file_round_trip_is_byte_stable(tmp_path, n):
    d = 32
    H, ids = _halves(n, d, 3), (np.arange(n, dtype=np.int64) * 7 + 5)
    fn = tmp_path / "a.faiss"
    faiss_io.write_idmap_sq16_ip(fn, H, ids)
    raw = fn.read_bytes()
    # the layout, restated: 'IxMp' + header, 'IxSQ' + header, the ScalarQuantizer record of 'IwSq' with qtype 4, codes, id map
    hdr = struct.pack("<iqqq?i", d, n, 1 << 20, 1 << 20, True, 0)
    want = (b"IxMp" + hdr + b"IxSQ" + hdr + struct.pack("<iifQQ", 4, 0, 0.0, d, 2 * d) + struct.pack("<Q", 0)
            + struct.pack("<Q", n * 2 * d) + H.astype("<f2").tobytes() + struct.pack("<Q", n) + ids.tobytes())
    assert raw == want
    assert faiss_io.index_fourcc(fn) == "IxMp" and faiss_io.index_fourcc(fn, inner=True) == "IxSQ" and faiss_io.index_ntotal(fn) == n
    for mmap in (True, False):
        H2, ids2 = faiss_io.read_idmap_sq16_ip(fn, mmap=mmap)
        assert H2.dtype == np.float16 and H2.shape == (n, d) and H2.tobytes() == H.tobytes() and np.array_equal(ids2, ids)
    st = faiss_io.read_index(fn)
    assert set(st) == {"halves", "ids"} and st["halves"].tobytes() == H.tobytes() and np.array_equal(st["ids"], ids)
    again = tmp_path / "b.faiss"
    faiss_io.write_index(again, st)
    assert again.read_bytes() == raw
    for lo, hi in ((0, n), (n // 3, n - n // 4), (n, n)):
        Hr, idr = faiss_io.read_idmap_sq16_ip_range(fn, lo, hi)
        assert Hr.tobytes() == H[lo:hi].tobytes() and np.array_equal(idr, ids[lo:hi])
        rr = faiss_io.read_index_range(fn, lo, hi)
        assert rr["halves"].tobytes() == H[lo:hi].tobytes() and np.array_equal(rr["ids"], ids[lo:hi])
    with pytest.raises(ValueError, match="outside"):
        faiss_io.read_idmap_sq16_ip_range(fn, 0, n + 1)
    # the halves keep what binary16 keeps: subnormals, signed zeros
    if n:
        H3 = H.copy()
        H3[0, :4] = np.array([6e-8, -6e-8, 0.0, -0.0], dtype=np.float16)
        faiss_io.write_idmap_sq16_ip(again, H3, ids)
        assert faiss_io.read_idmap_sq16_ip(again)[0].tobytes() == H3.tobytes()


def test_bare_record_reads_with_ids_equal_to_positions(tmp_path):
    n, d = 9, 16
    H = _halves(n, d, 4)
    hdr = struct.pack("<iqqq?i", d, n, 1 << 20, 1 << 20, True, 0)
    fn = tmp_path / "bare.faiss"
    fn.write_bytes(b"IxSQ" + hdr + struct.pack("<iifQQ", 4, 0, 0.0, d, 2 * d) + struct.pack("<Q", 0) + struct.pack("<Q", n * 2 * d)
                   + H.tobytes())
    H2, ids = faiss_io.read_idmap_sq16_ip(fn)
    assert H2.tobytes() == H.tobytes() and np.array_equal(ids, np.arange(n))
    assert faiss_io.index_fourcc(fn) == faiss_io.index_fourcc(fn, inner=True) == "IxSQ" and faiss_io.index_ntotal(fn) == n
    Hr, idr = faiss_io.read_idmap_sq16_ip_range(fn, 2, 6)
    assert Hr.tobytes() == H[2:6].tobytes() and np.array_equal(idr, np.arange(2, 6))


def test_corrupt_files_are_refused_by_name(tmp_path):
    n, d = 6, 16
    H, ids = _halves(n, d, 5), np.arange(n, dtype=np.int64)
    good = tmp_path / "good.faiss"
    faiss_io.write_idmap_sq16_ip(good, H, ids)
    raw = good.read_bytes()
    sq = 4 + 33 + 4 + 33                                                # where the ScalarQuantizer record starts
    cases = {
        "qtype": raw[:sq] + struct.pack("<i", 0) + raw[sq + 4:],
        "code_size": raw[:sq + 20] + struct.pack("<Q", d) + raw[sq + 28:],
        "d": raw[:sq + 12] + struct.pack("<Q", d + 16) + raw[sq + 20:],
        "trained": raw[:sq + 28] + struct.pack("<Q", 2) + raw[sq + 36:],
        "codes": raw[:sq + 36] + struct.pack("<Q", n * 2 * d - 2) + raw[sq + 44:],
        "outer_d": raw[:4] + struct.pack("<i", d + 16) + raw[8:],
    }
    for what, data in cases.items():
        fn = tmp_path / f"bad_{what}.faiss"
        fn.write_bytes(data)
        for call in (faiss_io.read_idmap_sq16_ip, faiss_io.index_ntotal, faiss_io.read_index, lambda p: faiss_io.read_idmap_sq16_ip_range(p, 0, 1)):
            with pytest.raises(RuntimeError, match=re.escape(str(fn))):
                call(fn)
    for cut in (2, 8 * n, 8 * n + 8, 8 * n + 8 + 5, len(raw) - 50, len(raw) - 10):
        fn = tmp_path / f"short_{cut}.faiss"
        fn.write_bytes(raw[:len(raw) - cut])
        with pytest.raises(RuntimeError, match=re.escape(str(fn))):
            faiss_io.read_idmap_sq16_ip(fn)
        with pytest.raises(RuntimeError, match=re.escape(str(fn))):
            faiss_io.read_idmap_sq16_ip_range(fn, n - 1, n)
    with pytest.raises(RuntimeError, match="No such file"):
        faiss_io.read_idmap_sq16_ip(tmp_path / "missing.faiss")
    # the fp32 flat file is not this record, and the fp32 reader does not take this one
    flat = tmp_path / "flat.faiss"
    faiss_io.write_idmap_flat_ip(flat, np.zeros((2, d), np.float32), np.arange(2))
    assert faiss_io.index_fourcc(flat, inner=True) == "IxFI"
    with pytest.raises(RuntimeError, match=re.escape(str(flat))):
        faiss_io.read_idmap_sq16_ip(flat)
    with pytest.raises(RuntimeError, match="expected IndexFlatIP"):
        faiss_io.read_idmap_flat_ip(good)


def test_the_fp32_flat_reader_shares_the_head_checks(tmp_path):
    """One parser reads the head of either flat file, so the fp32 reader refuses a file cut short by name as well, and reads a
    bare 'IxFI' record with ids equal to positions."""
    n, d = 6, 8
    X, ids = np.random.default_rng(6).standard_normal((n, d)).astype(np.float32), np.arange(n, dtype=np.int64) * 3 + 1
    good = tmp_path / "flat.faiss"
    faiss_io.write_idmap_flat_ip(good, X, ids)
    raw = good.read_bytes()
    for mmap in (True, False):
        X2, ids2 = faiss_io.read_idmap_flat_ip(good, mmap=mmap)
        assert X2.dtype == np.float32 and X2.tobytes() == X.tobytes() and np.array_equal(ids2, ids) and isinstance(X2, np.memmap) == mmap
    for cut in (2, 8 * n, 8 * n + 8, 8 * n + 8 + 5, len(raw) - 50, len(raw) - 10):
        fn = tmp_path / f"short_{cut}.faiss"
        fn.write_bytes(raw[:len(raw) - cut])
        with pytest.raises(RuntimeError, match=re.escape(str(fn))):
            faiss_io.read_idmap_flat_ip(fn)
    fn = tmp_path / "bad_count.faiss"
    fn.write_bytes(raw[:4 + 33 + 4 + 33] + struct.pack("<Q", n * d - 1) + raw[4 + 33 + 4 + 33 + 8:])
    with pytest.raises(RuntimeError, match="inconsistent flat payload"):
        faiss_io.read_idmap_flat_ip(fn)
    bare = tmp_path / "bare.faiss"
    bare.write_bytes(raw[4 + 33:len(raw) - 8 - 8 * n])                   # the 'IxFI' record alone
    Xb, idb = faiss_io.read_idmap_flat_ip(bare)
    assert Xb.tobytes() == X.tobytes() and np.array_equal(idb, np.arange(n))
    assert faiss_io.index_fourcc(bare, inner=True) == "IxFI" and faiss_io.index_fourcc(good, inner=True) == "IxFI"
    assert faiss_io.index_fourcc(good) == "IxMp"
    short = tmp_path / "head.faiss"
    short.write_bytes(raw[:4 + 20])                                      # ends inside the id map's header: no inner fourcc
    assert faiss_io.index_fourcc(short, inner=True) == "" and faiss_io.index_fourcc(short) == "IxMp"
    with pytest.raises(RuntimeError, match="is not IndexScalarQuantizer"):
        faiss_io.read_idmap_sq16_ip(good)
    other = tmp_path / "ivf.faiss"
    other.write_bytes(b"IwFl" + raw[4:])
    with pytest.raises(RuntimeError, match="not IndexIDMap/IndexFlatIP"):
        faiss_io.read_idmap_flat_ip(other)


# ---------------------------------------------------------------------------------------------------------------------
# a numpy stand-in for FlatSQfp16IPIndex: what FeatureSearchIndex.flat_sqfp16_index_factory must offer
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


class _CpuFlatSQ:
    """reserve / add_with_ids / add_halves_with_ids / search_device / search / range_search / remove_ids / reconstruct_batch /
    _selector_rows / rows_host (and merge_lists for the sharded wrapper): every answer by tests/sqfp16_flat_ref.py."""

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

    def hbm_bytes(self):
        return self.ntotal * (2 * self.d + 8)

    def _selector_rows(self):
        return torch.from_numpy(self.ids), 0, self.ntotal

    def rows_host(self):
        return self.H, self.ids

    def search_device(self, q, k, sel=None):
        Q = q.numpy()
        if sel is None:
            D, I = ref.topk(self.H, Q, k, ids=self.ids)
        else:
            D, I = ref.topk_pos(self.H, Q, k, np.flatnonzero(_selected(sel, self.ids)), ids=self.ids)
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

    @staticmethod
    def merge_lists(Ds, Is, k):
        from oracle import ip_topk_ref
        D, I = ip_topk_ref.merge_topk(Ds.numpy(), Is.numpy(), k)
        return torch.from_numpy(D), torch.from_numpy(I)


class _FakeTextTower:
    def __init__(self, d):
        self.d = d

    def extract_text_features(self, texts):
        import zlib
        out = np.stack([np.random.default_rng(zlib.crc32(t.encode())).standard_normal(self.d) for t in texts])
        return (out / np.linalg.norm(out, axis=1, keepdims=True)).astype(np.float32)


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
def test_type_name_is_parsed_and_the_refused_names_stay_refused(tmp_path):
    from wise_amd.index import feature_search_index as fsi
    from wise_amd.index.flat_sq import FlatSQfp16IPIndex

    assert "IndexSQfp16" in fsi.FLAT_TYPES and fsi._family(ITYPE) is None
    assert fsi.FeatureSearchIndex.flat_sqfp16_index_factory is FlatSQfp16IPIndex
    assert "IndexSQfp16" in fsi.__doc__ and "FlatSQfp16IPIndex" in fsi.__doc__
    _write_store(tmp_path / "features", unit_rows(12, 64, 9), np.arange(12) + 1)
    si = _factory(tmp_path)
    assert si.get_index_filename(ITYPE).name == "video-IndexSQfp16.faiss"
    old_prefix = ("IndexFlatIP, IndexIVFFlat and IndexIVFPQ<m> \\(with its R8 / R16 and IndexIVFOPQ<m> forms\\) and IndexIVFSQ8 are the "
                  "index types WISE builds, and IndexIVFSQfp16")
    for bad in ("IndexIVFSQ4", "IndexIVFSQ", "IndexIVFSQfp32", "IndexHNSW", "IndexHNSWFlat", "IndexOPQ64", "IndexSQ8", "IndexSQfp32", "IndexSQfp16 ",
                "indexsqfp16", "IndexFlatSQfp16"):
        with pytest.raises(NotImplementedError, match=re.escape(bad) + ": " + old_prefix + ".*IndexSQfp16"):
            si.create_index(bad)
        with pytest.raises(NotImplementedError, match=old_prefix):
            si.update_index(bad)
        assert not si.get_index_filename(bad).exists()
    with pytest.raises(FileNotFoundError, match="create_index"):
        si.update_index(ITYPE)
    _write_store(tmp_path / "b" / "features", unit_rows(12, 40, 9), np.arange(12) + 1)
    with pytest.raises(ValueError, match="multiple of 16"):
        _factory(tmp_path / "b").create_index(ITYPE)                     # refused before a row is read
    with pytest.raises(ValueError, match="multiple of 16"):
        FlatSQfp16IPIndex(40, device="cpu")
    # the sharded wrapper around the class keeps its refusals
    from wise_amd.index import sharded
    from wise_amd.index.selector import IDSelectorRange
    sh = sharded.ShardedFlatIPIndex(FlatSQfp16IPIndex(32, device="cpu"))
    assert sh.d == 32 and FlatSQfp16IPIndex.REMOVE_SCRATCH_BYTES == 64 << 20
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
    X, ids = unit_rows(N, d, 11), np.arange(N, dtype=np.int64) * 2 + 1
    X[200] = X[10]                                                       # equal rows: the lower position wins
    _write_store(tmp_path / "features", X, ids, per_file=64)
    monkeypatch.setattr(fsi.FeatureSearchIndex, "flat_sqfp16_index_factory", _CpuFlatSQ)
    monkeypatch.setattr(fsi, "FeatureExtractorFactory", lambda fid: _FakeTextTower(d))
    si = _factory(tmp_path)
    si.create_index(ITYPE)
    fn = si.get_index_filename(ITYPE)
    H = ref.encode(X)
    assert faiss_io.index_fourcc(fn, inner=True) == "IxSQ"
    Hf, idf = faiss_io.read_idmap_sq16_ip(fn)
    assert Hf.tobytes() == H.tobytes() and np.array_equal(idf, ids)      # the file holds numpy's cast of the store's rows
    before = fn.read_bytes()
    si.create_index(ITYPE)                                               # skip-if-exists
    assert fn.read_bytes() == before
    assert si.load_index(ITYPE) is True
    assert type(si.index) is _CpuFlatSQ and si.index.ntotal == N and si.index.reserved == N and si.index.H.tobytes() == H.tobytes()

    tower = _FakeTextTower(d)
    q = tower.extract_text_features(["This is a photo of a dog"])
    D1, I1 = ref.topk(H, q, 7, ids=ids)
    dist_, ids_ = si.search("video", "dog", topk=7)
    assert np.array_equal(ids_, I1[0]) and np.array_equal(dist_, D1[0])
    words = ["dog", "cat", "a red car", "rain"]
    Qb = tower.extract_text_features(["This is a photo of a " + w for w in words])
    Db, Ib = ref.topk(H, Qb, 5, ids=ids)
    got = si.search_batch("video", words, topk=5)
    assert len(got) == 4 and all(np.array_equal(g[0], Db[i]) and np.array_equal(g[1], Ib[i]) for i, g in enumerate(got))
    # within: an array of ids and a selector
    chosen = ids[5:60:3]
    Dw, Iw = ref.topk_pos(H, q, 7, np.flatnonzero(np.isin(ids, chosen)), ids=ids)
    dw, iw = si.search("video", "dog", topk=7, within=chosen)
    assert np.array_equal(iw, Iw[0]) and np.array_equal(dw, Dw[0]) and set(iw.tolist()) <= set(chosen.tolist())
    gw = si.search_batch("video", words, topk=5, within=IDSelectorRange(101, 301))
    in_range = np.flatnonzero((ids >= 101) & (ids < 301))
    Dr, Ir = ref.topk_pos(H, Qb, 5, in_range, ids=ids)
    assert all(np.array_equal(g[0], Dr[i]) and np.array_equal(g[1], Ir[i]) for i, g in enumerate(gw))
    # search_range: every row above the threshold, by descending score
    thr = float(np.sort(ref.scores(H, q)[0])[-20])
    lims, Dg, Ig = ref.range_search(H, q, thr, ids=ids)
    assert lims[1] == 19
    dr, ir = si.search_range("video", "dog", thr)
    assert np.array_equal(dr, Dg) and np.array_equal(ir, Ig) and (np.diff(dr) <= 0).all()
    dr2, ir2 = si.search_range("video", "dog", thr, within=chosen)
    keep = np.isin(ids, chosen)
    _, Dk, Ik = ref.range_search(H, q, thr, ids=ids, keep=keep)
    assert np.array_equal(dr2, Dk) and np.array_equal(ir2, Ik)

    # update_index: 40 vectors leave the store, 25 new ones arrive
    assert si.update_index(ITYPE) == (0, 0) and fn.read_bytes() == before
    rng = np.random.default_rng(12)
    gone = np.sort(rng.permutation(N)[:40])
    stay = np.setdiff1d(np.arange(N), gone)
    newX, new_ids = unit_rows(25, d, 13), np.arange(25, dtype=np.int64) + 5000
    import shutil
    shutil.rmtree(tmp_path / "features")
    order = rng.permutation(len(stay) + 25)                              # the store's own order: new rows anywhere
    sX, sid = np.concatenate([X[stay], newX])[order], np.concatenate([ids[stay], new_ids])[order]
    _write_store(tmp_path / "features", sX, sid, per_file=64)
    assert si.update_index(ITYPE) == (25, 40)
    H2, id2 = faiss_io.read_idmap_sq16_ip(fn)
    added = sid[np.isin(sid, new_ids)]                                   # in store order, behind the kept rows in their order
    assert np.array_equal(id2, np.concatenate([ids[stay], added]))
    assert H2.tobytes() == np.concatenate([H[stay], ref.encode(sX[np.isin(sid, new_ids)])]).tobytes()
    assert si.update_index(ITYPE) == (0, 0)
    assert si.load_index(ITYPE) is True and si.index.ntotal == N - 40 + 25
    D3, I3 = ref.topk(np.asarray(H2), q, 7, ids=id2)
    dist3, ids3 = si.search("video", "dog", topk=7)
    assert np.array_equal(ids3, I3[0]) and np.array_equal(dist3, D3[0])


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

    fsi.FeatureSearchIndex.flat_sqfp16_index_factory = _CpuFlatSQ
    fsi.FeatureExtractorFactory = lambda fid: _FakeTextTower(d)
    root = Path(root)
    Q = np.random.default_rng(6).standard_normal((3, d)).astype(np.float32)
    out = {}
    # (A) the single file a one-process create_index wrote: each rank takes rows shard_range(N, rank, world)
    # (B) the sharded build: every rank reads its own tar files only and writes its own part; load takes the part
    si2 = SearchIndexFactory("video", FID, {"features_dir": root / "features", "index_dir": root / "index_parts"})
    si2.create_index(ITYPE)
    part = si2.get_index_part_filename(ITYPE, rank, world)
    assert part.exists() and not si2.get_index_filename(ITYPE).exists() and faiss_io.index_fourcc(part, inner=True) == "IxSQ"
    dist.barrier()
    for tag, idir in (("A", root / "index_single"), ("B", root / "index_parts")):
        s = SearchIndexFactory("video", FID, {"features_dir": root / "features", "index_dir": idir})
        assert s.load_index(ITYPE) is True
        idx = s.index
        assert type(idx) is ShardedFlatIPIndex and type(idx.local) is _CpuFlatSQ and idx.ntotal == N
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
        out[f"{tag}_rec"] = idx.reconstruct_batch(np.array(WANT_IDS, dtype=np.int64))
    np.savez(root / f"sqfp16_rank{rank}.npz", **out)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_through_the_plugin_surface_world2(tmp_path):
    from wise_amd.index.search_index_factory import SearchIndexFactory
    from wise_amd.index.sharded import shard_range

    N, d, world = 1001, 32, 2
    X = unit_rows(N, d, 5)
    X[700] = X[20]                                                       # equal rows on both ranks' slices
    ids = np.arange(N, dtype=np.int64) + 1
    _write_store(tmp_path / "features", X, ids, per_file=100)           # 11 tar files: ranks get 6 and 5 of them
    single = SearchIndexFactory("video", FID, {"features_dir": tmp_path / "features", "index_dir": tmp_path / "index_single"})
    single.create_index(ITYPE)                                           # no process group here: the one-file build, no GPU needed
    H = ref.encode(X)
    assert faiss_io.read_idmap_sq16_ip(single.get_index_filename(ITYPE))[0].tobytes() == H.tobytes()
    mp.spawn(_plugin_worker, args=(world, _free_port(), str(tmp_path), N, d), nprocs=world, join=True)

    q = _FakeTextTower(d).extract_text_features(["This is a photo of a dog"])
    Q = np.random.default_rng(6).standard_normal((3, d)).astype(np.float32)
    D1, I1 = ref.topk(H, q, 7, ids=ids)
    D3, I3 = ref.topk(H, Q, 25, ids=ids)
    rec_ref = np.full((4, d), np.nan, np.float32)
    for i, w in enumerate(WANT_IDS):
        if w <= N:
            rec_ref[i] = H[w - 1].astype(np.float32)
    locals_ = []
    for r in range(world):
        g = np.load(tmp_path / f"sqfp16_rank{r}.npz")
        lo, hi = shard_range(N, r, world)
        assert np.array_equal(g["A_local_ids"], ids[lo:hi])
        for tag in "AB":
            assert np.array_equal(g[f"{tag}_ids"], I1[0]) and np.array_equal(g[f"{tag}_dist"], D1[0]), (r, tag)
            assert np.array_equal(g[f"{tag}_rec"], rec_ref, equal_nan=True), (r, tag)
        # (A) slices of the one file in its order: the answer is the whole index's, ties across the boundary included
        assert np.array_equal(g["A_I"], I3) and np.array_equal(g["A_D"], D3), r
        locals_.append(int(g["B_local"][0]))
        # a part holds the rank's own store shards, as halves
        part_ids = g["B_local_ids"]
        Hp, idp = faiss_io.read_idmap_sq16_ip(tmp_path / "index_parts" / f"video-{ITYPE}.faiss.part-{r:03d}-of-{world:03d}")
        assert np.array_equal(idp, part_ids) and Hp.tobytes() == H[part_ids - 1].tobytes()
    assert locals_ == [501, 500]                                         # tar files 0,2,..,10 (5 x 100 + the 1-row tail) and 1,3,..,9
    # (B) the parts are the store's shards dealt round-robin: the same rows in another order — the same scores, and the same ids
    # wherever the scores differ (rows 20 and 700 are equal: their order follows the parts')
    for r in range(world):
        g = np.load(tmp_path / f"sqfp16_rank{r}.npz")
        assert np.array_equal(g["B_D"], D3), r
        assert all(set(a.tolist()) == set(b.tolist()) for a, b in zip(g["B_I"], I3)), r


# ---------------------------------------------------------------------------------------------------------------------
# the recorded quality study
def test_recorded_quality_study_first_seed_and_the_derived_bound():
    gold = json.loads((ROOT / "tests" / "golden" / "sqfp16_flat_quality.json").read_text())
    assert gold["seeds"] == [0, 1, 2, 3, 4] and json.dumps(ref.STUDY) in gold["what"] and len(gold["runs"]) == 5
    assert ref.STUDY["rows"] == 60000 and ref.STUDY["dim"] == 128 and ref.STUDY["k"] == 10
    run = ref.quality_study(gold["seeds"][0])
    assert run == gold["runs"][0], (run, gold["runs"][0])
    assert gold["recall_min"] == min(r["recall"] for r in gold["runs"])
    assert gold["max_abs_score_gap"] == max(r["max_abs_score_gap"] for r in gold["runs"])
    for r in gold["runs"]:
        # the bound is computed from the data (sqfp16_flat_ref.error_bound), per query; no query exceeds its own
        assert r["gap_over_bound_max"] <= 1.0 and r["max_abs_score_gap"] <= r["bound"], r
        assert 0.0 < r["max_abs_score_gap"] and r["recall"] >= 0.99, r

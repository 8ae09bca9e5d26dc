"""CPU tests (-m "not gpu") of IndexSQ8bit: the entry points are declared, exported and bound; the index file ('IxMp' around 'IxSQ'
with a QT_8bit record); the type's name in the plugin; the plugin's build over a numpy stand-in for FlatSQ8IPIndex, in one process
and at world size 2 (gloo); and the recorded quality and band studies.  The kernels themselves: tests/test_gpu_sq8_flat.py."""
import json
import os
import re
import shutil
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

import sq8_flat_ref as ref  # noqa: E402
from wise_amd import _lib  # noqa: E402
from wise_amd.index import faiss_io  # noqa: E402

ITYPE = "IndexSQ8bit"
FID = "mlfoundations/open_clip/ViT-B-32/seeded-0"
FMAX = 3.4028234663852886e38
# entry point -> number of arguments
NEW_SYMBOLS = {"wise_ipsq8_topk": 14, "wise_ipsq8_topk_pos": 16, "wise_ipsq8_range_count": 12, "wise_ipsq8_range_fill": 15,
               "wise_ipsq8_reconstruct": 10, "wise_ipsq8_prepare": 5, "wise_ipsq8_topk_batched": 16, "wise_sq_minmax": 7}
NEW_SIZES = {"wise_ipsq8_topk_workspace_bytes": 4, "wise_ipsq8_range_workspace_bytes": 3, "wise_ipsq8_topk_batched_workspace_bytes": 4}


def unit_rows(n, d, seed):
    X = np.random.default_rng(seed).standard_normal((n, d))
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
def test_entry_points_declared_exported_and_bound():
    from wise_amd.build import HIP_SOURCES, CSRC, declared_symbols

    declared = set(declared_symbols())
    assert set(_lib.SIGNATURES) == declared
    assert "ip_sq8.hip" in HIP_SOURCES and (CSRC / "ip_sq8.hip").exists()
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
    assert "wise_ipsq8_" in header.split("int wise_abi_version(void);")[0]           # listed as added within 5
    integration = (ROOT / "INTEGRATION.md").read_text()
    for name in list(NEW_SYMBOLS) + list(NEW_SIZES):
        assert name in integration, name


def test_workspace_functions_answer_without_a_device():
    lib = _lib.load()
    assert lib.wise_ipsq8_topk_workspace_bytes(1000, 64, 4, 10) > 0
    assert lib.wise_ipsq8_topk_workspace_bytes(0, 64, 1, 10) > 0                    # an empty index is searched: all padding
    # W and q0 stand in front of what the shared scan uses: the sibling's size (one scan, one plan) plus their room
    for N, d, nq, k in ((1000, 64, 4, 10), (100000, 512, 5, 100), (0, 16, 1, 1)):
        head = -(-nq * d * 4 // 256) * 256 + -(-nq * 4 // 256) * 256
        assert lib.wise_ipsq8_topk_workspace_bytes(N, d, nq, k) == head + lib.wise_ipsqfp16_topk_workspace_bytes(N, d, nq, k)
    for N, d, nq, k in ((1000, 20, 1, 10), (1000, 8, 1, 10), (1000, 1040, 1, 10), (1000, 64, 0, 10), (1000, 64, 1025, 10),
                        (1000, 64, 1, 0), (1000, 64, 1, 2049), (-1, 64, 1, 10)):
        assert lib.wise_ipsq8_topk_workspace_bytes(N, d, nq, k) == 0, (N, d, nq, k)
    assert lib.wise_ipsq8_range_workspace_bytes(5000, 64, 3) > 0 and lib.wise_ipsq8_range_workspace_bytes(0, 64, 3) > 0
    for N, d, nq in ((5000, 20, 3), (5000, 64, 0), (5000, 64, 65536), (-1, 64, 3)):
        assert lib.wise_ipsq8_range_workspace_bytes(N, d, nq) == 0, (N, d, nq)
    # the batched search: d % 128 == 0 in [256, 1024], nq >= 3, k <= 128, N >= 4096 — and NO large-N floor beyond that
    for d in (256, 384, 512, 768, 1024):
        assert lib.wise_ipsq8_topk_batched_workspace_bytes(4096, d, 3, 128) > 0
        assert lib.wise_ipsq8_topk_batched_workspace_bytes(40000, d, 130, 10) > 0
    for N, d, nq, k in ((4095, 512, 64, 10), (40000, 512, 2, 10), (40000, 512, 64, 129), (40000, 128, 64, 10), (40000, 320, 64, 10),
                        (40000, 20, 64, 10), (1 << 31, 512, 64, 10)):
        assert lib.wise_ipsq8_topk_batched_workspace_bytes(N, d, nq, k) == 0, (N, d, nq, k)


# ---------------------------------------------------------------------------------------------------------------------
# the file
def _codes(n, d, seed):
    X = unit_rows(max(n, 1), d, seed)
    vmin, vdiff = ref.train(X)
    return np.concatenate([vmin, vdiff]), ref.encode(X[:n], vmin, vdiff)


@pytest.mark.parametrize("n", [0, 1, 77])
def test_file_round_trip_is_byte_stable(tmp_path, n):
    d = 32
    (trained, C), ids = _codes(n, d, 3), (np.arange(n, dtype=np.int64) * 7 + 5)
    fn = tmp_path / "a.faiss"
    faiss_io.write_idmap_sq8_ip(fn, trained, C, ids)
    raw = fn.read_bytes()
    # the layout, restated: 'IxMp' + header, 'IxSQ' + header, the ScalarQuantizer record with qtype 0 and its 2d trained floats, the
    # codes, the id map
    hdr = struct.pack("<iqqq?i", d, n, 1 << 20, 1 << 20, True, 0)
    want = (b"IxMp" + hdr + b"IxSQ" + hdr + struct.pack("<iifQQ", 0, 0, 0.0, d, d) + struct.pack("<Q", 2 * d) + trained.astype("<f4").tobytes()
            + struct.pack("<Q", n * d) + C.tobytes() + struct.pack("<Q", n) + ids.tobytes())
    assert raw == want
    assert faiss_io.index_fourcc(fn) == "IxMp" and faiss_io.index_fourcc(fn, inner=True) == "IxSQ" and faiss_io.index_ntotal(fn) == n
    assert faiss_io.flat_sq_qtype(fn) == 0 and faiss_io.idmap_sq8_ip_ntotal(fn) == n
    for mmap in (True, False):
        t2, C2, ids2 = faiss_io.read_idmap_sq8_ip(fn, mmap=mmap)
        assert C2.dtype == np.uint8 and C2.shape == (n, d) and C2.tobytes() == C.tobytes() and np.array_equal(ids2, ids)
        assert t2.dtype == np.float32 and t2.tobytes() == trained.tobytes() and isinstance(C2, np.memmap) == (mmap and n > 0)
    st = faiss_io.read_index(fn)
    assert set(st) == {"trained", "codes", "ids"} and st["codes"].tobytes() == C.tobytes() and np.array_equal(st["ids"], ids)
    again = tmp_path / "b.faiss"
    faiss_io.write_index(again, st)
    assert again.read_bytes() == raw
    for lo, hi in ((0, n), (n // 3, n - n // 4), (n, n)):
        tr, Cr, idr = faiss_io.read_idmap_sq8_ip_range(fn, lo, hi)
        assert Cr.tobytes() == C[lo:hi].tobytes() and np.array_equal(idr, ids[lo:hi]) and tr.tobytes() == trained.tobytes()
        rr = faiss_io.read_index_range(fn, lo, hi)
        assert rr["codes"].tobytes() == C[lo:hi].tobytes() and np.array_equal(rr["ids"], ids[lo:hi]) and rr["trained"].tobytes() == trained.tobytes()
    with pytest.raises(ValueError, match="outside"):
        faiss_io.read_idmap_sq8_ip_range(fn, 0, n + 1)
    # a bare 'IxSQ' record reads with ids equal to positions
    bare = tmp_path / "bare.faiss"
    bare.write_bytes(raw[4 + 33:len(raw) - 8 - 8 * n])
    tb, Cb, idb = faiss_io.read_idmap_sq8_ip(bare)
    assert Cb.tobytes() == C.tobytes() and np.array_equal(idb, np.arange(n)) and tb.tobytes() == trained.tobytes()
    assert faiss_io.flat_sq_qtype(bare) == 0 and faiss_io.index_ntotal(bare) == n


def test_corrupt_files_are_refused_by_name_and_the_two_records_stay_apart(tmp_path):
    n, d = 6, 16
    (trained, C), ids = _codes(n, d, 5), np.arange(n, dtype=np.int64)
    good = tmp_path / "good.faiss"
    faiss_io.write_idmap_sq8_ip(good, trained, C, ids)
    raw = good.read_bytes()
    sq = 4 + 33 + 4 + 33                                                # where the ScalarQuantizer record starts
    pay = sq + 36 + 8 * d                                               # where the codes' length stands
    cases = {
        "qtype": raw[:sq] + struct.pack("<i", 4) + raw[sq + 4:],        # says QT_fp16 over this payload
        "qtype1": raw[:sq] + struct.pack("<i", 1) + raw[sq + 4:],       # QT_4bit
        "code_size": raw[:sq + 20] + struct.pack("<Q", 2 * d) + raw[sq + 28:],
        "d": raw[:sq + 12] + struct.pack("<Q", d + 16) + raw[sq + 20:],
        "trained": raw[:sq + 28] + struct.pack("<Q", 0) + raw[sq + 36:],
        "trained_d": raw[:sq + 28] + struct.pack("<Q", d) + raw[sq + 36:],
        "codes": raw[:pay] + struct.pack("<Q", n * d - 2) + raw[pay + 8:],
        "outer_d": raw[:4] + struct.pack("<i", d + 16) + raw[8:],
    }
    for what, data in cases.items():
        fn = tmp_path / f"bad_{what}.faiss"
        fn.write_bytes(data)
        for call in (faiss_io.read_idmap_sq8_ip, faiss_io.idmap_sq8_ip_ntotal, faiss_io.index_ntotal, faiss_io.read_index,
                     lambda p: faiss_io.read_idmap_sq8_ip_range(p, 0, 1), faiss_io.read_idmap_sq16_ip):
            with pytest.raises(RuntimeError, match=re.escape(str(fn))):
                call(fn)
    for cut in (2, 8 * n, 8 * n + 8, 8 * n + 8 + 5, len(raw) - pay - 4, len(raw) - sq - 40, len(raw) - 50, len(raw) - 10):
        fn = tmp_path / f"short_{cut}.faiss"
        fn.write_bytes(raw[:len(raw) - cut])
        with pytest.raises(RuntimeError, match=re.escape(str(fn))):
            faiss_io.read_idmap_sq8_ip(fn)
        with pytest.raises(RuntimeError, match=re.escape(str(fn))):
            faiss_io.read_idmap_sq8_ip_range(fn, n - 1, n)
    with pytest.raises(RuntimeError, match="No such file"):
        faiss_io.read_idmap_sq8_ip(tmp_path / "missing.faiss")
    # a qtype-4 file is not read as this type, and the reverse; the fp32 flat file is neither
    half = tmp_path / "half.faiss"
    faiss_io.write_idmap_sq16_ip(half, np.zeros((n, d), np.float16), ids)
    assert faiss_io.flat_sq_qtype(half) == 4 and set(faiss_io.read_index(half)) == {"halves", "ids"}
    with pytest.raises(RuntimeError, match=re.escape(str(half))):
        faiss_io.read_idmap_sq8_ip(half)
    with pytest.raises(RuntimeError, match=re.escape(str(good))):
        faiss_io.read_idmap_sq16_ip(good)
    with pytest.raises(RuntimeError, match=re.escape(str(good))):
        faiss_io.idmap_sq16_ip_ntotal(good)
    flat = tmp_path / "flat.faiss"
    faiss_io.write_idmap_flat_ip(flat, np.zeros((2, d), np.float32), np.arange(2))
    assert faiss_io.flat_sq_qtype(flat) is None
    with pytest.raises(RuntimeError, match=re.escape(str(flat))):
        faiss_io.read_idmap_sq8_ip(flat)
    with pytest.raises(RuntimeError, match="expected IndexFlatIP"):
        faiss_io.read_idmap_flat_ip(good)


# ---------------------------------------------------------------------------------------------------------------------
# a numpy stand-in for FlatSQ8IPIndex: what FeatureSearchIndex.flat_sq8_index_factory must offer
def _selected(sel, ids):
    from wise_amd.index.selector import IDSelectorBatch, IDSelectorNot, IDSelectorRange
    if isinstance(sel, IDSelectorBatch):
        return np.isin(ids, sel.ids)
    if isinstance(sel, IDSelectorRange):
        return (ids >= sel.imin) & (ids < sel.imax)
    if isinstance(sel, IDSelectorNot):
        return ~_selected(sel.sel, ids)
    raise TypeError(type(sel).__name__)


class _CpuFlatSQ8:
    """minmax / set_minmax / set_trained / trained_host / reserve / add_with_ids / add_codes_with_ids / search_device / search /
    range_search / remove_ids / reconstruct_batch / _selector_rows / rows_host (and merge_lists for the sharded wrapper): every answer
    by tests/sq8_flat_ref.py."""

    def __init__(self, d):
        self.d, self.device = int(d), torch.device("cpu")
        self.C, self.ids = np.zeros((0, d), np.uint8), np.zeros(0, np.int64)
        self.is_trained = False

    def minmax(self, x, lohi=None):
        x = np.asarray(x, np.float32)
        if lohi is None:
            lohi = torch.tensor([[FMAX] * self.d, [-FMAX] * self.d], dtype=torch.float32)
        if len(x):
            lohi[0] = torch.minimum(lohi[0], torch.from_numpy(x.min(axis=0)))
            lohi[1] = torch.maximum(lohi[1], torch.from_numpy(x.max(axis=0)))
        return lohi

    def set_minmax(self, lohi):
        lohi = lohi.numpy().astype(np.float32)
        if (lohi[0] > lohi[1]).any():
            lohi = np.zeros_like(lohi)
        self.set_trained(lohi[0], (lohi[1] - lohi[0]).astype(np.float32))

    def set_trained(self, vmin, vdiff):
        self.vmin, self.vdiff = np.asarray(vmin, np.float32).copy(), np.asarray(vdiff, np.float32).copy()
        self.is_trained = True

    def trained_host(self):
        return self.vmin, self.vdiff

    def reserve(self, n):
        self.reserved = int(n)

    def add_with_ids(self, x, ids):
        assert self.is_trained
        self.add_codes_with_ids(ref.encode(np.asarray(x, np.float32), self.vmin, self.vdiff), ids)

    def add_codes_with_ids(self, c, ids):
        assert self.is_trained and np.asarray(c).dtype == np.uint8
        self.C = np.concatenate([self.C, np.asarray(c)])
        self.ids = np.concatenate([self.ids, np.asarray(ids, np.int64)])

    @property
    def ntotal(self):
        return self.C.shape[0]

    def hbm_bytes(self):
        return self.ntotal * (self.d + 8) + 8 * self.d

    def _selector_rows(self):
        return torch.from_numpy(self.ids), 0, self.ntotal

    def rows_host(self):
        return self.C, self.ids

    def _scores(self, Q):
        return ref.scores(self.C, self.vmin, self.vdiff, Q)

    def search_device(self, q, k, sel=None):
        S = self._scores(q.numpy())
        if sel is None:
            D, I = ref.topk(S, k, ids=self.ids)
        else:
            D, I = ref.topk_pos(S, k, np.flatnonzero(_selected(sel, self.ids)), ids=self.ids)
        return torch.from_numpy(D), torch.from_numpy(I)

    def search(self, x, k, params=None):
        D, I = self.search_device(torch.from_numpy(np.ascontiguousarray(x, np.float32)), k, None if params is None else params.sel)
        return D.numpy(), I.numpy()

    def range_search(self, x, thresh, params=None):
        keep = None if params is None or params.sel is None else _selected(params.sel, self.ids)
        return ref.range_search(self._scores(np.ascontiguousarray(x, np.float32)), thresh, ids=self.ids, keep=keep)

    def remove_ids(self, sel):
        from wise_amd.index.selector import as_selector
        gone = _selected(as_selector(sel), self.ids)
        self.C, self.ids = self.C[~gone], self.ids[~gone]
        return int(gone.sum())

    def reconstruct_batch(self, want):
        return ref.reconstruct(self.C, self.vmin, self.vdiff, self.ids, want)

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
    from wise_amd.index.flat_sq import FlatSQ8IPIndex

    assert ITYPE in fsi.FLAT_TYPES and fsi._family(ITYPE) is None and fsi.FLAT_TYPES[ITYPE].trained
    assert [t for t, f in fsi.FLAT_TYPES.items() if f.trained] == [ITYPE]
    assert fsi.FeatureSearchIndex.flat_sq8_index_factory is FlatSQ8IPIndex
    assert ITYPE in fsi.__doc__ and "FlatSQ8IPIndex" in fsi.__doc__
    _write_store(tmp_path / "features", unit_rows(12, 64, 9), np.arange(12) + 1)
    si = _factory(tmp_path)
    assert si.get_index_filename(ITYPE).name == "video-IndexSQ8bit.faiss"
    old_prefix = ("IndexFlatIP, IndexIVFFlat and IndexIVFPQ<m> \\(with its R8 / R16 and IndexIVFOPQ<m> forms\\) and IndexIVFSQ8 are the "
                  "index types WISE builds, and IndexIVFSQfp16")
    for bad in ("IndexSQ8", "IndexSQ8bit ", "indexsq8bit", "IndexSQ4bit", "IndexSQ8bit_uniform", "IndexFlatSQ8", "IndexSQfp32", "IndexHNSW"):
        with pytest.raises(NotImplementedError, match=re.escape(bad) + ": " + old_prefix + ", and IndexSQ8bit, and IndexSQfp16, and IndexFlatL2$"):
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
        FlatSQ8IPIndex(40, device="cpu")
    idx = FlatSQ8IPIndex(32, device="cpu")                               # training state, without a device
    assert not idx.is_trained and idx.hbm_bytes() == 8 * 32 and FlatSQ8IPIndex.BATCH_MIN_QUERIES == 8 and FlatSQ8IPIndex.BATCH_MIN_ROWS == 1 << 18
    with pytest.raises(RuntimeError, match="before train"):
        idx.add_with_ids(np.zeros((2, 32), np.float32), np.arange(2))
    with pytest.raises(RuntimeError, match="before train"):
        idx.add_codes_with_ids(np.zeros((2, 32), np.uint8), np.arange(2))
    with pytest.raises(ValueError, match="32 values"):
        idx.set_trained(np.zeros(16, np.float32), np.zeros(32, np.float32))
    idx.set_trained(np.arange(32, dtype=np.float32), np.ones(32, np.float32))
    assert idx.is_trained and np.array_equal(idx.trained_host()[0], np.arange(32, dtype=np.float32))
    idx.add_codes_with_ids(np.full((3, 32), 7, np.uint8), np.arange(3))
    assert idx.ntotal == 3 and idx.hbm_bytes() == 3 * 40 + 256 and idx.rows_host()[0].dtype == np.uint8
    with pytest.raises(RuntimeError, match="cannot change"):
        idx.set_trained(np.zeros(32, np.float32), np.ones(32, np.float32))
    from wise_amd.index import sharded
    from wise_amd.index.selector import IDSelectorRange
    sh = sharded.ShardedFlatIPIndex(FlatSQ8IPIndex(32, device="cpu"))
    assert sh.d == 32
    with pytest.raises(NotImplementedError, match="no selector"):
        sh.search_device(None, 5, sel=IDSelectorRange(0, 10))


# ---------------------------------------------------------------------------------------------------------------------
# the plugin in one process
def test_plugin_create_load_search_update_with_a_stand_in(tmp_path, monkeypatch):
    from wise_amd.index import feature_search_index as fsi
    from wise_amd.index.selector import IDSelectorRange

    N, d = 300, 32
    X, ids = unit_rows(N, d, 11), np.arange(N, dtype=np.int64) * 2 + 1
    X[200] = X[10]                                                       # equal rows: the lower position wins
    _write_store(tmp_path / "features", X, ids, per_file=64)
    monkeypatch.setattr(fsi.FeatureSearchIndex, "flat_sq8_index_factory", _CpuFlatSQ8)
    monkeypatch.setattr(fsi, "FeatureExtractorFactory", lambda fid: _FakeTextTower(d))
    si = _factory(tmp_path)
    si.create_index(ITYPE)
    fn = si.get_index_filename(ITYPE)
    vmin, vdiff = ref.train(X)                                           # the ranges over EVERY row of the store: nothing clamps
    C = ref.encode(X, vmin, vdiff)
    assert faiss_io.index_fourcc(fn, inner=True) == "IxSQ" and faiss_io.flat_sq_qtype(fn) == 0
    tf, Cf, idf = faiss_io.read_idmap_sq8_ip(fn)
    assert Cf.tobytes() == C.tobytes() and np.array_equal(idf, ids) and tf.tobytes() == np.concatenate([vmin, vdiff]).tobytes()
    assert np.abs(ref.decode(C, vmin, vdiff) - X).max() <= vdiff.max() / 510 * 1.001          # every row within half a bin
    before = fn.read_bytes()
    si.create_index(ITYPE)                                               # skip-if-exists
    assert fn.read_bytes() == before
    assert si.load_index(ITYPE) is True
    assert type(si.index) is _CpuFlatSQ8 and si.index.ntotal == N and si.index.reserved == N and si.index.C.tobytes() == C.tobytes()
    assert si.index.vmin.tobytes() == vmin.tobytes() and si.index.vdiff.tobytes() == vdiff.tobytes()

    tower = _FakeTextTower(d)
    q = tower.extract_text_features(["This is a photo of a dog"])
    S = ref.scores(C, vmin, vdiff, q)
    D1, I1 = ref.topk(S, 7, ids=ids)
    dist_, ids_ = si.search("video", "dog", topk=7)
    assert np.array_equal(ids_, I1[0]) and np.array_equal(dist_, D1[0])
    words = ["dog", "cat", "a red car", "rain"]
    Qb = tower.extract_text_features(["This is a photo of a " + w for w in words])
    Sb = ref.scores(C, vmin, vdiff, Qb)
    Db, Ib = ref.topk(Sb, 5, ids=ids)
    got = si.search_batch("video", words, topk=5)
    assert len(got) == 4 and all(np.array_equal(g[0], Db[i]) and np.array_equal(g[1], Ib[i]) for i, g in enumerate(got))
    chosen = ids[5:60:3]
    Dw, Iw = ref.topk_pos(S, 7, np.flatnonzero(np.isin(ids, chosen)), ids=ids)
    dw, iw = si.search("video", "dog", topk=7, within=chosen)
    assert np.array_equal(iw, Iw[0]) and np.array_equal(dw, Dw[0])
    gw = si.search_batch("video", words, topk=5, within=IDSelectorRange(101, 301))
    Dr, Ir = ref.topk_pos(Sb, 5, np.flatnonzero((ids >= 101) & (ids < 301)), ids=ids)
    assert all(np.array_equal(g[0], Dr[i]) and np.array_equal(g[1], Ir[i]) for i, g in enumerate(gw))
    thr = float(np.sort(S[0])[-20])
    lims, Dg, Ig = ref.range_search(S, thr, ids=ids)
    dr, ir = si.search_range("video", "dog", thr)
    assert lims[1] == 19 and np.array_equal(dr, Dg) and np.array_equal(ir, Ig) and (np.diff(dr) <= 0).all()
    rec = si.index.reconstruct_batch(np.array([ids[3], 4], dtype=np.int64))
    assert np.array_equal(rec[0], ref.decode(C[3:4], vmin, vdiff)[0]) and np.isnan(rec[1]).all()

    # update_index: 40 vectors leave the store, 25 new ones arrive, some outside the ranges AS TRAINED: they clamp, the ranges stay
    assert si.update_index(ITYPE) == (0, 0) and fn.read_bytes() == before
    rng = np.random.default_rng(12)
    gone = np.sort(rng.permutation(N)[:40])
    stay = np.setdiff1d(np.arange(N), gone)
    newX, new_ids = unit_rows(25, d, 13) * np.float32(1.5), np.arange(25, dtype=np.int64) + 5000
    assert (newX > vmin + vdiff).any() or (newX < vmin).any()
    shutil.rmtree(tmp_path / "features")
    order = rng.permutation(len(stay) + 25)                              # the store's own order: new rows anywhere
    sX, sid = np.concatenate([X[stay], newX])[order], np.concatenate([ids[stay], new_ids])[order]
    _write_store(tmp_path / "features", sX, sid, per_file=64)
    assert si.update_index(ITYPE) == (25, 40)
    t2, C2, id2 = faiss_io.read_idmap_sq8_ip(fn)
    added = sid[np.isin(sid, new_ids)]                                   # in store order, behind the kept rows in their order
    assert np.array_equal(id2, np.concatenate([ids[stay], added])) and t2.tobytes() == tf.tobytes()
    assert C2.tobytes() == np.concatenate([C[stay], ref.encode(sX[np.isin(sid, new_ids)], vmin, vdiff)]).tobytes()
    assert si.update_index(ITYPE) == (0, 0)
    assert si.load_index(ITYPE) is True and si.index.ntotal == N - 40 + 25
    D3, I3 = ref.topk(ref.scores(np.asarray(C2), vmin, vdiff, q), 7, ids=id2)
    dist3, ids3 = si.search("video", "dog", topk=7)
    assert np.array_equal(ids3, I3[0]) and np.array_equal(dist3, D3[0])


# ---------------------------------------------------------------------------------------------------------------------
# the plugin at world size 2 (gloo): the collective build — ranges all-reduced, the skip decision taken together
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _plugin_worker(rank, world, port, root, N, d):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import wise_amd.index.feature_search_index as fsi
    from wise_amd.index.search_index_factory import SearchIndexFactory
    from wise_amd.index.sharded import ShardedFlatIPIndex, shard_range

    fsi.FeatureSearchIndex.flat_sq8_index_factory = _CpuFlatSQ8
    fsi.FeatureExtractorFactory = lambda fid: _FakeTextTower(d)
    root = Path(root)
    Q = np.random.default_rng(6).standard_normal((3, d)).astype(np.float32)
    out = {}
    si2 = SearchIndexFactory("video", FID, {"features_dir": root / "features", "index_dir": root / "index_parts"})
    part = si2.get_index_part_filename(ITYPE, rank, world)
    # rank 0 already has a part (a stale one) and rank 1 has none: the decision is collective, so rank 0 does not leave rank 1 alone
    # in the all-reduce of the ranges — both build, and the stale part is replaced
    assert part.exists() == (rank == 0)
    stale = part.read_bytes() if rank == 0 else None
    si2.create_index(ITYPE)
    assert part.exists() and not si2.get_index_filename(ITYPE).exists() and faiss_io.flat_sq_qtype(part) == 0
    assert stale is None or part.read_bytes() != stale
    dist.barrier()
    built = part.read_bytes()
    si2.create_index(ITYPE)                                              # every rank has its part now: all skip, together
    assert part.read_bytes() == built
    # a store of one shard file: rank 1's slice is empty — it contributes +max / -max and writes an empty part with the same ranges
    si3 = SearchIndexFactory("video", FID, {"features_dir": root / "features_one", "index_dir": root / "index_one"})
    si3.create_index(ITYPE)
    t3, C3, _ = faiss_io.read_idmap_sq8_ip(si3.get_index_part_filename(ITYPE, rank, world))
    out["one_trained"], out["one_rows"] = t3, np.array([C3.shape[0]])
    dist.barrier()
    for tag, idir in (("A", root / "index_single"), ("B", root / "index_parts")):
        s = SearchIndexFactory("video", FID, {"features_dir": root / "features", "index_dir": idir})
        assert s.load_index(ITYPE) is True
        idx = s.index
        assert type(idx) is ShardedFlatIPIndex and type(idx.local) is _CpuFlatSQ8 and idx.ntotal == N and idx.local.is_trained
        if tag == "A":
            lo, hi = shard_range(N, rank, world)
            assert idx.local.ntotal == hi - lo and idx.local.reserved == hi - lo
        with pytest.raises(NotImplementedError):
            s.update_index(ITYPE)
        out[f"{tag}_trained"] = np.concatenate(idx.local.trained_host())
        out[f"{tag}_local_ids"] = idx.local.ids
        out[f"{tag}_dist"], out[f"{tag}_ids"] = s.search("video", "dog", topk=7)
        out[f"{tag}_D"], out[f"{tag}_I"] = idx.search(Q, 25)
        out[f"{tag}_rec"] = idx.reconstruct_batch(np.array([1, 1001, 500, 1006], dtype=np.int64))
    np.savez(root / f"sq8_rank{rank}.npz", **out)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_build_and_load_through_the_plugin_surface_world2(tmp_path, monkeypatch):
    from wise_amd.index import feature_search_index as fsi
    from wise_amd.index.sharded import shard_range

    N, d, world = 1001, 32, 2
    X = unit_rows(N, d, 5)
    X[700] = X[20]                                                       # equal rows on both ranks' slices
    X[3, 4], X[998, 9] = np.float32(2.0), np.float32(-2.0)               # the extremes of two dimensions, on different ranks' shards
    ids = np.arange(N, dtype=np.int64) + 1
    _write_store(tmp_path / "features", X, ids, per_file=100)           # 11 tar files: ranks get 6 and 5 of them
    _write_store(tmp_path / "features_one", X[:50], ids[:50], per_file=100)       # one tar file: rank 1 gets none
    monkeypatch.setattr(fsi.FeatureSearchIndex, "flat_sq8_index_factory", _CpuFlatSQ8)
    from wise_amd.index.search_index_factory import SearchIndexFactory
    single = SearchIndexFactory("video", FID, {"features_dir": tmp_path / "features", "index_dir": tmp_path / "index_single"})
    single.create_index(ITYPE)                                           # no process group here: the one-file build
    vmin, vdiff = ref.train(X)
    trained = np.concatenate([vmin, vdiff])
    C = ref.encode(X, vmin, vdiff)
    t1, C1, id1 = faiss_io.read_idmap_sq8_ip(single.get_index_filename(ITYPE))
    assert C1.tobytes() == C.tobytes() and t1.tobytes() == trained.tobytes() and np.array_equal(id1, ids)
    (tmp_path / "index_parts").mkdir()
    stale = tmp_path / "index_parts" / f"video-{ITYPE}.faiss.part-000-of-002"
    faiss_io.write_idmap_sq8_ip(stale, np.zeros(2 * d, np.float32), np.zeros((1, d), np.uint8), np.array([77]))
    mp.spawn(_plugin_worker, args=(world, _free_port(), str(tmp_path), N, d), nprocs=world, join=True)

    q = _FakeTextTower(d).extract_text_features(["This is a photo of a dog"])
    Q = np.random.default_rng(6).standard_normal((3, d)).astype(np.float32)
    D1, I1 = ref.topk(ref.scores(C, vmin, vdiff, q), 7, ids=ids)
    D3, I3 = ref.topk(ref.scores(C, vmin, vdiff, Q), 25, ids=ids)
    rec_ref = ref.reconstruct(C, vmin, vdiff, ids, [1, 1001, 500, 1006])
    v1, vd1 = ref.train(X[:50])
    got_ids, got_codes, rows = [], [], []
    for r in range(world):
        g = np.load(tmp_path / f"sq8_rank{r}.npz")
        lo, hi = shard_range(N, r, world)
        assert np.array_equal(g["A_local_ids"], ids[lo:hi])
        for tag in "AB":
            assert g[f"{tag}_trained"].tobytes() == trained.tobytes(), (r, tag)          # every rank holds the one-process ranges
            assert np.array_equal(g[f"{tag}_ids"], I1[0]) and np.array_equal(g[f"{tag}_dist"], D1[0]), (r, tag)
            assert np.array_equal(g[f"{tag}_rec"], rec_ref, equal_nan=True), (r, tag)
        assert np.array_equal(g["A_I"], I3) and np.array_equal(g["A_D"], D3), r
        assert np.array_equal(g["B_D"], D3) and all(set(a.tolist()) == set(b.tolist()) for a, b in zip(g["B_I"], I3)), r
        tp, Cp, idp = faiss_io.read_idmap_sq8_ip(tmp_path / "index_parts" / f"video-{ITYPE}.faiss.part-{r:03d}-of-{world:03d}")
        assert tp.tobytes() == trained.tobytes() and np.array_equal(idp, g["B_local_ids"])
        got_ids.append(idp)
        got_codes.append(np.asarray(Cp))
        assert g["one_trained"].tobytes() == np.concatenate([v1, vd1]).tobytes()         # the empty rank holds the ranges too
        rows.append(int(g["one_rows"][0]))
    assert rows == [50, 0] and [len(i) for i in got_ids] == [501, 500]
    # the parts' codes, brought into the single file's order by their ids, are the single file's codes
    all_ids, all_codes = np.concatenate(got_ids), np.concatenate(got_codes)
    order = np.argsort(all_ids)
    assert np.array_equal(all_ids[order], ids) and all_codes[order].tobytes() == C.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# the recorded studies
def test_recorded_quality_study_first_seed_and_the_derived_bound():
    gold = json.loads((ROOT / "tests" / "golden" / "sq8_flat_quality.json").read_text())
    assert gold["seeds"] == [0, 1, 2, 3, 4] and json.dumps(ref.STUDY) in gold["what"] and len(gold["runs"]) == 5
    assert ref.STUDY["rows"] == 60000 and ref.STUDY["dim"] == 128 and ref.STUDY["k"] == 10
    run = ref.quality_study(gold["seeds"][0])
    assert run == gold["runs"][0], (run, gold["runs"][0])
    assert gold["recall_min"] == min(r["recall"] for r in gold["runs"])
    assert gold["max_abs_score_gap"] == max(r["max_abs_score_gap"] for r in gold["runs"])
    for r in gold["runs"]:
        # the bound is computed from the data (sq8_flat_ref.error_bound), per query; no query exceeds its own
        assert r["gap_over_bound_max"] <= 1.0 and 0.0 < r["max_abs_score_gap"] <= r["bound"], r
        assert r["recall"] >= gold["recall_min"] and 0.0 < r["recall"] <= 1.0, r


def test_recorded_band_study():
    gold = json.loads((ROOT / "tests" / "golden" / "sq8_flat_band.json").read_text())
    assert json.dumps(ref.BAND) in gold["what"] and [r["dim"] for r in gold["runs"]] == ref.BAND["dims"] == [256, 1024]
    assert ref.BAND["rows"] == 40000 and ref.BAND["queries"] == 64 and ref.BAND["cap"] == 4096
    for r in gold["runs"]:
        assert 0.0 < r["error_over_band_max"] <= 1.0, r                  # no query's collect error leaves its band
        assert r["missed"] == 0 and 0 < r["longest_list"] < 1024, r      # and the lists stay under a quarter of their slots
    # the image and the band of a few weight rows, recomputed: scaling keeps every weight out of binary16's subnormal range
    W = np.random.default_rng(0).standard_normal((4, 256)).astype(np.float32) * np.float32(1e-6)
    e, image, eps = ref.query_image(W)
    mx = np.abs(np.ldexp(W.astype(np.float64), e[:, None])).max(axis=1)
    assert ((mx >= 2.0 ** 14) & (mx < 2.0 ** 15)).all() and (eps > 0).all()
    assert np.abs(image).max() < 65504 and (np.abs(W) < 2.0 ** -14).all()

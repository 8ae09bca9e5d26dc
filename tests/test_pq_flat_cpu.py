"""CPU tests (-m "not gpu") of IndexPQ<m> and its R8 / R16 forms: the entry points are declared, exported and bound and refuse what
they do not serve; the two index files ('IxMp' around 'IxPq', and 'WiFR' around it); the types' names in the plugin; the plugin's
build, load, update and search over a numpy stand-in for the two classes; and the recorded recall study.  The kernels themselves:
tests/test_gpu_pq_flat.py."""
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

import ivfpq_ref  # noqa: E402
import ivfpq_refine_ref  # noqa: E402
import pq_flat_ref as ref  # noqa: E402
from wise_amd import _lib  # noqa: E402
from wise_amd.index import faiss_io  # noqa: E402

FID = "mlfoundations/open_clip/ViT-B-32/seeded-0"
NEW_SYMBOLS = {"wise_pqflat_topk": 13, "wise_pqflat_topk_pos": 15, "wise_pqflat_decode": 9}      # entry point -> number of arguments
NEW_SIZES = {"wise_pqflat_topk_workspace_bytes": 4}
UNKNOWN = ("IndexFlatIP, IndexIVFFlat and IndexIVFPQ<m> \\(with its R8 / R16 and IndexIVFOPQ<m> forms\\) and IndexIVFSQ8 are the "
           "index types WISE builds, and IndexIVFSQfp16, and IndexSQ8bit, and IndexSQfp16, and IndexFlatL2$")


def unit_rows(n, d, seed):
    X = np.random.default_rng(seed).standard_normal((n, d))
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
def test_entry_points_declared_exported_and_bound():
    from wise_amd.build import HIP_SOURCES, CSRC, declared_symbols

    declared = set(declared_symbols())
    assert set(_lib.SIGNATURES) == declared
    assert "pq_flat.hip" in HIP_SOURCES and (CSRC / "pq_flat.hip").exists()
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
    assert "wise_pqflat_" in header.split("int wise_abi_version(void);")[0]           # listed as added within 5
    assert "THE SCORE IS A CONTRACT: acc = +0.0f" in header                           # the header states the contract
    integration = (ROOT / "INTEGRATION.md").read_text()
    for name in list(NEW_SYMBOLS) + list(NEW_SIZES):
        assert name in integration, name


def test_workspace_function_answers_without_a_device():
    lib = _lib.load()
    ws = lib.wise_pqflat_topk_workspace_bytes
    assert ws(1000, 64, 4, 10) > 0
    assert ws(0, 64, 1, 10) > 0                                         # an empty index is searched: all padding
    assert ws(1000, 64, 0, 10) > 0 and ws(1000, 64, 100000, 10) == ws(1000, 64, 1000, 10)      # nq of any size: the call makes the passes
    for m in (1, 4, 8, 12, 16, 20, 48, 64, 128):
        for k in (1, 10, 100, 2048):
            assert ws(20011, m, 9, k) > 0, (m, k)
    assert ws(2 ** 32 - 2, 128, 1, 2048) > 0
    for N, m, nq, k in ((1000, 0, 1, 10), (1000, 129, 1, 10), (1000, -1, 1, 10), (1000, 64, -1, 10), (1000, 64, 1, 0), (1000, 64, 1, 2049),
                        (-1, 64, 1, 10), (2 ** 32 - 1, 64, 1, 10)):
        assert ws(N, m, nq, k) == 0, (N, m, nq, k)
    # more rows never take less room, and the room is bounded by what is resident at once (no growth with N past a full grid)
    assert ws(100, 16, 4, 10) <= ws(10 ** 6, 16, 4, 10) == ws(10 ** 9, 16, 4, 10)


def test_host_side_refusals_of_the_entry_points_need_no_device():
    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.uint8)
    p = buf.data_ptr()
    for m, k in ((0, 10), (129, 10), (16, 0), (16, 2049)):
        assert lib.wise_pqflat_topk(p, 10, m, p, 1, k, 0, 0, p, p, p, 4096, 0) == -3
        assert lib.wise_pqflat_topk_pos(p, 10, m, p, 5, p, 1, k, 0, 0, p, p, p, 4096, 0) == -3
        assert b"unsupported" in lib.wise_last_error()
    assert lib.wise_pqflat_topk(p, 2 ** 32 - 1, 16, p, 1, 10, 0, 0, p, p, p, 4096, 0) == -3
    assert lib.wise_pqflat_topk(p, 10, 16, p, 1, 10, 0, 0, p, p, p, 16, 0) == -2          # a short workspace
    assert lib.wise_pqflat_topk(p, 10, 16, p, 1, 10, 0, 0, p, p, 0, 0, 0) == -2
    assert lib.wise_pqflat_topk(p, 10, 16, 0, 1, 10, 0, 0, p, p, p, 4096, 0) == -1         # a null table
    assert lib.wise_pqflat_topk_pos(p, 10, 16, p, 11, p, 1, 10, 0, 0, p, p, p, 4096, 0) == -1      # more positions than rows
    assert lib.wise_pqflat_topk_pos(p, 10, 16, 0, 5, p, 1, 10, 0, 0, p, p, p, 4096, 0) == -1       # null positions
    assert lib.wise_pqflat_decode(p, 10, p, 1, p, 64, 7, p, 0) == -3 and lib.wise_pqflat_decode(p, 10, p, 1, p, 64, 129, p, 0) == -3
    assert lib.wise_pqflat_decode(p, 10, p, 1, 0, 64, 8, p, 0) == -1
    assert not buf.any()


# ---------------------------------------------------------------------------------------------------------------------
# the files
def _state(n, d, m, seed, kind=None):
    rng = np.random.default_rng(seed)
    st = dict(codebooks=rng.standard_normal((m, 256, d // m)).astype(np.float32), codes=rng.integers(0, 256, (n, m)).astype(np.uint8),
              ids=np.arange(n, dtype=np.int64) * 7 + 5)
    if kind is not None:
        rows, scales = ivfpq_refine_ref.quantise(rng.standard_normal((n, d)).astype(np.float32), kind)
        st.update(kind=kind, k_factor=50 if kind == 8 else 20, rows=rows, scales=scales)
    return st


def _plain_bytes(st):
    """the 'IxMp' / 'IxPq' layout, restated"""
    (n, m), d = st["codes"].shape, st["codebooks"].shape[0] * st["codebooks"].shape[2]
    hdr = struct.pack("<iqqq?i", d, n, 1 << 20, 1 << 20, True, 0)
    return (b"IxMp" + hdr + b"IxPq" + hdr + struct.pack("<QQQQ", d, m, 8, 256 * d) + st["codebooks"].astype("<f4").tobytes()
            + struct.pack("<Q", n * m) + st["codes"].tobytes() + struct.pack("<iBi", 0, 0, 8 * m + 1) + struct.pack("<Q", n) + st["ids"].tobytes())


def _equal_state(a, b):
    if set(a) != set(b):
        return False
    for key in a:
        x, y = a[key], b[key]
        if x is None or y is None or np.isscalar(x):
            if not (x is None and y is None) and x != y:
                return False
        elif np.asarray(x).dtype != np.asarray(y).dtype or np.asarray(x).tobytes() != np.asarray(y).tobytes():
            return False
    return True


@pytest.mark.parametrize("n", [0, 1, 77])
def test_file_round_trips_are_byte_stable_and_their_digests_are_recorded(tmp_path, n, golden_dir):
    d, m = 32, 4
    gold = json.loads((golden_dir / "pq_flat_file_digests.json").read_text())
    for kind in (None, 8, 16):
        st = _state(n, d, m, 3 + n, kind)
        fn = tmp_path / f"a{kind}.faiss"
        faiss_io.write_index(fn, st)
        raw = fn.read_bytes()
        plain = _plain_bytes(st)
        if kind is None:
            want = plain
        else:
            want = struct.pack("<4sIII", b"WiFR", 1, kind, st["k_factor"]) + plain + struct.pack("<Q", st["rows"].nbytes) + st["rows"].tobytes()
            if kind == 8:
                want += struct.pack("<Q", n) + st["scales"].tobytes()
        assert raw == want
        assert hashlib.sha256(raw).hexdigest() == gold[f"n={n} d={d} m={m} kind={kind}"]
        assert faiss_io.index_fourcc(fn) == ("IxMp" if kind is None else "WiFR") and faiss_io.index_ntotal(fn) == n
        assert faiss_io.index_fourcc(fn, inner=True) == ("IxPq" if kind is None else "WiFR")
        reader = faiss_io.read_idmap_pq_ip if kind is None else faiss_io.read_pq_refine_ip
        for mmap in (True, False):
            got = reader(fn, mmap=mmap)
            assert _equal_state(got, st) and isinstance(got["codes"], np.memmap) == (mmap and n > 0)
        assert _equal_state(faiss_io.read_index(fn), st)
        again = tmp_path / "b.faiss"
        faiss_io.write_index(again, faiss_io.read_index(fn))
        assert again.read_bytes() == raw
        for lo, hi in ((0, n), (n // 3, n - n // 4), (n, n)):
            part = faiss_io.read_index_range(fn, lo, hi)
            cut = {key: (v[lo:hi] if key in ("codes", "ids", "rows", "scales") and v is not None else v) for key, v in st.items()}
            assert _equal_state(part, cut), (lo, hi)
        with pytest.raises(ValueError, match="outside"):
            faiss_io.read_index_range(fn, 0, n + 1)
    # a bare 'IxPq' record reads with ids equal to positions
    st = _state(n, d, m, 3 + n)
    raw = _plain_bytes(st)
    bare = tmp_path / "bare.faiss"
    bare.write_bytes(raw[4 + 33:len(raw) - 8 - 8 * n])
    got = faiss_io.read_idmap_pq_ip(bare)
    assert got["codes"].tobytes() == st["codes"].tobytes() and np.array_equal(got["ids"], np.arange(n)) and faiss_io.index_ntotal(bare) == n


def test_corrupt_and_foreign_files_are_refused_by_name(tmp_path):
    n, d, m = 6, 16, 4
    st = _state(n, d, m, 5)
    good = tmp_path / "good.faiss"
    faiss_io.write_index(good, st)
    raw = good.read_bytes()
    pq = 4 + 33 + 4 + 33                                                # where the ProductQuantizer record starts
    pay = pq + 32 + 4 * 256 * d                                         # where the codes' length stands
    cases = {
        "nbits": raw[:pq + 16] + struct.pack("<Q", 4) + raw[pq + 24:],
        "n_floats": raw[:pq + 24] + struct.pack("<Q", 128 * d) + raw[pq + 32:],
        "d": raw[:pq] + struct.pack("<Q", d + 4) + raw[pq + 8:],
        "m": raw[:pq + 8] + struct.pack("<Q", 5) + raw[pq + 16:],
        "n_bytes": raw[:pay] + struct.pack("<Q", n * m - 2) + raw[pay + 8:],
        "outer_d": raw[:4] + struct.pack("<i", d + 16) + raw[8:],
        "outer_n": raw[:8] + struct.pack("<q", n + 1) + raw[16:],
        "metric": raw[:4 + 33 + 4 + 29] + struct.pack("<i", 1) + raw[pq:],
        "id_map": raw[:len(raw) - 8 * n - 8] + struct.pack("<Q", n - 1) + raw[len(raw) - 8 * n:],
    }
    for what, data in cases.items():
        fn = tmp_path / f"bad_{what}.faiss"
        fn.write_bytes(data)
        for call in (faiss_io.read_idmap_pq_ip, faiss_io.read_index, lambda p: faiss_io.read_index_range(p, 0, 1)):
            with pytest.raises(RuntimeError, match=re.escape(str(fn))):
                call(fn)
        if what != "id_map":                                            # (the id map lies behind what the head reads)
            with pytest.raises(RuntimeError, match=re.escape(str(fn))):
                faiss_io.index_ntotal(fn)
    for cut in (2, 8 * n, 8 * n + 8, 8 * n + 8 + 5, len(raw) - pay - 4, len(raw) - pq - 40, len(raw) - pq - 10, len(raw) - 50, len(raw) - 10):
        fn = tmp_path / f"short_{cut}.faiss"
        fn.write_bytes(raw[:len(raw) - cut])
        with pytest.raises(RuntimeError, match=re.escape(str(fn))):
            faiss_io.read_idmap_pq_ip(fn)
        with pytest.raises(RuntimeError, match=re.escape(str(fn))):
            faiss_io.read_idmap_pq_ip_range(fn, n - 1, n)
    with pytest.raises(RuntimeError, match="No such file"):
        faiss_io.read_idmap_pq_ip(tmp_path / "missing.faiss")
    # the 'WiFR' wrapper: head, rows and scales
    for kind in (8, 16):
        str_ = _state(n, d, m, 6, kind)
        fr = tmp_path / f"fr{kind}.faiss"
        faiss_io.write_index(fr, str_)
        rr = fr.read_bytes()
        rows_at = 16 + len(_plain_bytes(str_))
        bad = {"version": rr[:4] + struct.pack("<I", 2) + rr[8:], "kind": rr[:8] + struct.pack("<I", 4) + rr[12:],
               "k_factor": rr[:12] + struct.pack("<I", 0) + rr[16:], "rows": rr[:rows_at] + struct.pack("<Q", 3) + rr[rows_at + 8:],
               "inner_n_bytes": rr[:16 + pay] + struct.pack("<Q", n * m + 1) + rr[16 + pay + 8:], "cut": rr[:-3], "cut_head": rr[:10],
               "cut_rows": rr[:rows_at + 4]}
        if kind == 8:
            bad["scales"] = rr[:len(rr) - 4 * n - 8] + struct.pack("<Q", n + 1) + rr[len(rr) - 4 * n:]
        for what, data in bad.items():
            fn = tmp_path / f"fr{kind}_{what}.faiss"
            fn.write_bytes(data)
            for call in (faiss_io.read_pq_refine_ip, faiss_io.read_index, lambda p: faiss_io.read_index_range(p, 0, 1)):
                with pytest.raises(RuntimeError, match=re.escape(str(fn))):
                    call(fn)
        with pytest.raises(RuntimeError, match=re.escape(str(fr))):
            faiss_io.read_idmap_pq_ip(fr)                               # the wrapper is not the plain record
        with pytest.raises(RuntimeError, match=re.escape(str(good))):
            faiss_io.read_pq_refine_ip(good)                            # and the reverse
    # the other flat readers do not take this file, and this reader none of theirs
    for other in (faiss_io.read_idmap_flat_ip, faiss_io.read_idmap_sq16_ip, faiss_io.read_idmap_sq8_ip, faiss_io.read_idmap_flat_l2):
        with pytest.raises(RuntimeError, match=re.escape(str(good))):
            other(good)
    flat = tmp_path / "flat.faiss"
    faiss_io.write_idmap_flat_ip(flat, np.zeros((2, d), np.float32), np.arange(2))
    with pytest.raises(RuntimeError, match=re.escape(str(flat))):
        faiss_io.read_idmap_pq_ip(flat)


def test_files_of_the_existing_types_are_dispatched_as_before(tmp_path):
    n, d = 5, 16
    ids = np.arange(n, dtype=np.int64)
    half, sq8, ivf = tmp_path / "half.faiss", tmp_path / "sq8.faiss", tmp_path / "ivf.faiss"
    faiss_io.write_idmap_sq16_ip(half, np.zeros((n, d), np.float16), ids)
    faiss_io.write_idmap_sq8_ip(sq8, np.zeros(2 * d, np.float32), np.zeros((n, d), np.uint8), ids)
    st = _state(n, d, 4, 1)
    faiss_io.write_index(ivf, dict(st, centroids=np.zeros((2, d), np.float32), list_off=np.array([0, 2, n], dtype=np.int64)))
    assert set(faiss_io.read_index(half)) == {"halves", "ids"} and set(faiss_io.read_index(sq8)) == {"trained", "codes", "ids"}
    assert faiss_io.index_fourcc(ivf) == "IwPQ" and set(faiss_io.read_index(ivf)) == {"centroids", "codebooks", "codes", "ids", "list_off", "nprobe"}
    assert faiss_io.index_ntotal(half) == faiss_io.index_ntotal(sq8) == faiss_io.index_ntotal(ivf) == n
    fr = tmp_path / "ivfr.faiss"
    faiss_io.write_index(fr, dict(_state(n, d, 4, 1, 8), centroids=np.zeros((2, d), np.float32), list_off=np.array([0, 2, n], dtype=np.int64)))
    assert faiss_io.index_fourcc(fr) == "WiPR" and faiss_io.read_index(fr)["kind"] == 8
    flat = tmp_path / "flat.faiss"
    faiss_io.write_idmap_flat_ip(flat, np.zeros((2, d), np.float32), np.arange(2))
    with pytest.raises(RuntimeError, match="is not an inverted-file index"):
        faiss_io.read_index(flat)
    with pytest.raises(TypeError, match="no record"):
        faiss_io.write_index(flat, {"ids": ids, "list_off": np.array([0, n])})


# ---------------------------------------------------------------------------------------------------------------------
# a numpy stand-in for the two classes: what FeatureSearchIndex.flat_pq_index_factory / flat_pq_refine_index_factory must offer
def _selected(sel, ids):
    from wise_amd.index.selector import IDSelectorBatch, IDSelectorNot, IDSelectorRange
    if isinstance(sel, IDSelectorBatch):
        return np.isin(ids, sel.ids)
    if isinstance(sel, IDSelectorRange):
        return (ids >= sel.imin) & (ids < sel.imax)
    if isinstance(sel, IDSelectorNot):
        return ~_selected(sel.sel, ids)
    raise TypeError(type(sel).__name__)


class _CpuFlatPQ:
    """train / set_codebooks / reserve / add_with_ids / add_codes_with_ids / search / remove_ids / _selector_rows / state_host: every
    answer by tests/pq_flat_ref.py (the float64 trainer of ivfpq_ref: the stand-in is not held to the GPU trainer's bits)."""
    kind = None

    def __init__(self, d, m):
        self.d, self.m, self.device = int(d), int(m), torch.device("cpu")
        self.codes, self.ids, self.codebooks = np.zeros((0, m), np.uint8), np.zeros(0, np.int64), None
        self.X = np.zeros((0, d), np.float32)
        self.trained_on = None

    def train(self, x):
        x = np.asarray(x, np.float32)
        self.trained_on = x.shape[0]
        self.codebooks = ivfpq_ref.train(x[ivfpq_ref.training_rows(x.shape[0], 1234)], self.m, niter=2).astype(np.float32)

    def set_codebooks(self, cb):
        self.codebooks = np.asarray(cb, np.float32).copy()

    def reserve(self, n):
        self.reserved = int(n)

    def add_with_ids(self, x, ids):
        assert self.codebooks is not None
        x = np.asarray(x, np.float32)
        self._extra(x)
        self.add_codes_with_ids(ivfpq_ref.encode(x, self.codebooks), ids)

    def _extra(self, x):
        pass

    def add_codes_with_ids(self, c, ids):
        assert self.codebooks is not None and np.asarray(c).dtype == np.uint8
        self.codes = np.concatenate([self.codes, np.asarray(c)])
        self.ids = np.concatenate([self.ids, np.asarray(ids, np.int64)])

    @property
    def ntotal(self):
        return self.codes.shape[0]

    def _selector_rows(self):
        return torch.from_numpy(self.ids), 0, self.ntotal

    def search(self, x, k, params=None):
        lut = ivfpq_ref.lut(np.asarray(x, np.float32), self.codebooks).astype(np.float32)
        if params is None or params.sel is None:
            return ref.scan(self.codes, self.ids, lut, k)
        return ref.scan_pos(self.codes, self.ids, lut, np.flatnonzero(_selected(params.sel, self.ids)), k)

    def remove_ids(self, sel):
        from wise_amd.index.selector import as_selector
        gone = _selected(as_selector(sel), self.ids)
        self._drop(gone)
        self.codes, self.ids = self.codes[~gone], self.ids[~gone]
        return int(gone.sum())

    def _drop(self, gone):
        pass

    def state_host(self):
        return dict(codebooks=self.codebooks, codes=self.codes, ids=self.ids)


class _CpuFlatPQRefine(_CpuFlatPQ):
    def __init__(self, d, m, kind, k_factor=50):
        super().__init__(d, m)
        self.kind, self.k_factor = kind, k_factor
        self.rows = np.zeros((0, d), np.int8 if kind == 8 else np.uint16)
        self.scales = np.zeros(0, np.float32) if kind == 8 else None

    def _extra(self, x):
        rows, scales = ivfpq_refine_ref.quantise(x, self.kind)
        self.rows = np.concatenate([self.rows, rows])
        if self.kind == 8:
            self.scales = np.concatenate([self.scales, scales])

    def add_codes_with_ids(self, c, ids, rows=None, scales=None):
        if rows is not None:
            self.rows = np.concatenate([self.rows, np.asarray(rows)])
            if self.kind == 8:
                self.scales = np.concatenate([self.scales, np.asarray(scales)])
        super().add_codes_with_ids(c, ids)

    def _drop(self, gone):
        self.rows = self.rows[~gone]
        if self.kind == 8:
            self.scales = self.scales[~gone]

    def search(self, x, k, params=None):
        x = np.asarray(x, np.float32)
        lut = ivfpq_ref.lut(x, self.codebooks).astype(np.float32)
        pos = None if params is None or params.sel is None else np.flatnonzero(_selected(params.sel, self.ids))
        return ref.search_refine(self.codes, self.ids, lut, self.rows, self.kind, self.scales, x, k, self.k_factor, pos=pos)

    def state_host(self):
        return dict(super().state_host(), kind=self.kind, k_factor=self.k_factor, rows=self.rows, scales=self.scales)


class _FakeTextTower:
    def __init__(self, d):
        self.d = d

    def extract_text_features(self, texts):
        import zlib
        out = np.stack([np.random.default_rng(zlib.crc32(t.encode())).standard_normal(self.d) for t in texts])
        return (out / np.linalg.norm(out, axis=1, keepdims=True)).astype(np.float32)


def _write_store(fdir, X, ids, per_file=2048):
    import shutil
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    shutil.rmtree(fdir, ignore_errors=True)
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
# names and shapes
def test_type_names_are_parsed_and_the_refused_names_stay_refused(tmp_path):
    from wise_amd.index import feature_search_index as fsi
    from wise_amd.index.flat_pq import FlatPQIPIndex, FlatPQRefineIPIndex

    assert fsi.parse_pq_flat_type("IndexPQ64") == (64, None) and fsi.parse_pq_flat_type("IndexPQ8R8") == (8, 8)
    assert fsi.parse_pq_flat_type("IndexPQ128R16") == (128, 16) and fsi.parse_pq_flat_type("IndexPQ1") == (1, None)
    for name in ("IndexPQ64", "IndexPQ64R8", "IndexPQ64R16"):
        assert name not in fsi.FLAT_TYPES and fsi._family(name) is None
    assert "IndexPQ<m>" in fsi.__doc__ and "IndexPQ<m>R16" in fsi.__doc__
    assert [t for t, f in fsi.FLAT_TYPES.items() if f.trained] == ["IndexSQ8bit"]      # the new types are not entries of that table
    assert fsi.FeatureSearchIndex.flat_pq_index_factory is FlatPQIPIndex
    assert fsi.FeatureSearchIndex.flat_pq_refine_index_factory is FlatPQRefineIPIndex
    assert "FlatPQIPIndex" in fsi.__doc__ and "FlatPQRefineIPIndex" in fsi.__doc__ and "IndexPQ<m>R8" in fsi.__doc__
    _write_store(tmp_path / "features", unit_rows(12, 64, 9), np.arange(12) + 1)
    si = _factory(tmp_path)
    assert si.get_index_filename("IndexPQ8R16").name == "video-IndexPQ8R16.faiss"
    for bad in ("IndexPQ", "IndexPQ0", "IndexPQ064", "IndexPQ64R4", "IndexPQ64 ", "indexpq64", "IndexOPQ64", "IndexPQ64\n", "IndexPQR8",
                "IndexPQ64R", "IndexPQ64R08"):
        assert fsi.parse_pq_flat_type(bad) is None, bad
        with pytest.raises(NotImplementedError, match=re.escape(bad) + ": " + UNKNOWN):
            si.create_index(bad)
        with pytest.raises(NotImplementedError, match=re.escape(bad) + ": " + UNKNOWN):
            si.update_index(bad)
        assert not si.get_index_filename(bad).exists()
    with pytest.raises(FileNotFoundError, match="create_index"):
        si.update_index("IndexPQ8")


def test_shapes_are_refused_before_a_row_is_read(tmp_path, monkeypatch):
    from wise_amd.index import feature_search_index as fsi
    from wise_amd.index.flat_pq import FlatPQIPIndex, FlatPQRefineIPIndex

    def no_rows(store):
        raise AssertionError("a row was read")

    _write_store(tmp_path / "features", unit_rows(12, 60, 9), np.arange(12) + 1)
    si = _factory(tmp_path)
    monkeypatch.setattr(fsi, "_read_store", no_rows)
    for name, what in (("IndexPQ7", "not a multiple"), ("IndexPQ129", r"out of \[1, 128\]"), ("IndexPQ20", "must be even"),
                       ("IndexPQ6R8", "multiple of 16"), ("IndexPQ6R16", "multiple of 8")):
        with pytest.raises(ValueError, match=what):
            si.create_index(name)
        assert not si.get_index_filename(name).exists()
    for d, m in ((60, 7), (64, 129), (60, 20)):
        with pytest.raises(ValueError):
            FlatPQIPIndex(d, m, device="cpu")
    with pytest.raises(ValueError, match="multiple of 16"):
        FlatPQRefineIPIndex(24, 4, 8, device="cpu")
    with pytest.raises(ValueError, match="kind=4"):
        FlatPQRefineIPIndex(32, 4, 4, device="cpu")
    # the classes' host-side state, without a device
    idx = FlatPQIPIndex(32, 4, device="cpu")
    assert not idx.is_trained and idx.ntotal == 0 and idx.hbm_bytes() == 4 * 256 * 32 and idx.m == 4 and idx.dsub == 8
    for early in (lambda: idx.add_with_ids(np.zeros((2, 32), np.float32), np.arange(2)),
                  lambda: idx.add_codes_with_ids(np.zeros((2, 4), np.uint8), np.arange(2)), lambda: idx.state_host()):
        with pytest.raises(RuntimeError, match="before train"):
            early()
    with pytest.raises(ValueError, match="training vectors"):
        idx.train(np.zeros((255, 32), np.float32))
    with pytest.raises(ValueError, match=r"expected \[4,256,8\]"):
        idx.set_codebooks(np.zeros((4, 256, 4), np.float32))
    cb = np.random.default_rng(0).standard_normal((4, 256, 8)).astype(np.float32)
    idx.set_codebooks(cb)
    idx.add_codes_with_ids(np.full((3, 4), 7, np.uint8), np.arange(3) + 10)
    assert idx.is_trained and idx.ntotal == 3 and idx.hbm_bytes() == 3 * 12 + 4 * 256 * 32
    with pytest.raises(ValueError, match=r"expected \[n,4\]"):
        idx.add_codes_with_ids(np.zeros((2, 32), np.uint8), np.arange(2))
    with pytest.raises(RuntimeError, match="cannot change"):
        idx.set_codebooks(cb)
    with pytest.raises(NotImplementedError):
        idx.range_search(np.zeros((1, 32), np.float32), 0.5)
    st = idx.state_host()
    assert set(st) == {"codebooks", "codes", "ids"} and st["codes"].tobytes() == bytes([7] * 12) and np.array_equal(st["ids"], [10, 11, 12])
    r8 = FlatPQRefineIPIndex(32, 4, 8, k_factor=9, device="cpu")
    r8.set_codebooks(cb)
    assert r8.candidates(10) == 90 and r8.candidates(300) == 2048 and FlatPQRefineIPIndex(32, 4, 16, device="cpu").k_factor == 50
    with pytest.raises(ValueError, match="compact rows"):
        r8.add_codes_with_ids(np.zeros((2, 4), np.uint8), np.arange(2))
    r8.add_codes_with_ids(np.zeros((2, 4), np.uint8), np.arange(2), rows=np.ones((2, 32), np.int8), scales=np.ones(2, np.float32))
    st = r8.state_host()
    assert st["kind"] == 8 and st["k_factor"] == 9 and st["rows"].shape == (2, 32) and st["scales"].shape == (2,)
    assert r8.hbm_bytes() == 2 * (12 + 36) + 4 * 256 * 32


# ---------------------------------------------------------------------------------------------------------------------
# the plugin in one process, over the stand-ins
@pytest.mark.parametrize("itype", ["IndexPQ8", "IndexPQ8R8", "IndexPQ8R16"])
def test_plugin_create_load_search_update_with_a_stand_in(tmp_path, monkeypatch, itype):
    from wise_amd.index import feature_search_index as fsi

    kind = {"IndexPQ8": None, "IndexPQ8R8": 8, "IndexPQ8R16": 16}[itype]
    N, d, m = 600, 64, 8
    X, ids = unit_rows(N, d, 3), np.arange(N, dtype=np.int64) * 3 + 2
    _write_store(tmp_path / "features", X, ids, per_file=256)
    made = []

    def plain(d_, m_):
        made.append(_CpuFlatPQ(d_, m_))
        return made[-1]

    def refine(d_, m_, kind_, k_factor=50):
        made.append(_CpuFlatPQRefine(d_, m_, kind_, k_factor))
        return made[-1]

    monkeypatch.setattr(fsi.FeatureSearchIndex, "flat_pq_index_factory", staticmethod(plain))
    monkeypatch.setattr(fsi.FeatureSearchIndex, "flat_pq_refine_index_factory", staticmethod(refine))
    monkeypatch.setattr(fsi, "FeatureExtractorFactory", lambda fid: _FakeTextTower(d))
    si = _factory(tmp_path)
    si.create_index(itype)
    fn = si.get_index_filename(itype)
    built = made[-1]
    assert built.trained_on == fsi._training_plan(N)[1] and built.reserved == N and built.ntotal == N
    f = faiss_io.read_index(fn)
    assert f["codes"].tobytes() == ivfpq_ref.encode(X, built.codebooks).tobytes() and np.array_equal(f["ids"], ids)
    assert f["codebooks"].tobytes() == built.codebooks.tobytes() and f.get("kind") == kind
    size = fn.stat().st_size
    si.create_index(itype)                                              # skip-if-exists
    assert fn.stat().st_size == size and made[-1] is built
    assert si.load_index(itype) is True and si.is_index_loaded()
    loaded = si.index
    assert loaded is made[-1] and loaded is not built and loaded.ntotal == N and loaded.reserved == N
    assert _equal_state(loaded.state_host(), built.state_host())
    dist, got = si.search("video", "dog", topk=5)
    q = _FakeTextTower(d).extract_text_features(["This is a photo of a dog"])
    Dw, Iw = built.search(q, 5)
    assert np.array_equal(got, Iw[0]) and np.array_equal(dist, Dw[0])
    inside = ids[100:140]
    dist, got = si.search("video", "dog", topk=5, within=inside)
    assert np.isin(got, inside).all() and (np.diff(dist) <= 0).all()
    # update_index: 50 vectors leave, 30 arrive at the end of the store; codebooks and k_factor stay
    rng = np.random.default_rng(8)
    gone = np.sort(rng.permutation(N)[:50])
    stay = np.setdiff1d(np.arange(N), gone)
    newX, new_ids = unit_rows(30, d, 4), np.arange(30, dtype=np.int64) + 10 ** 6
    X2, ids2 = np.concatenate([X[stay], newX]), np.concatenate([ids[stay], new_ids])
    _write_store(tmp_path / "features", X2, ids2, per_file=256)
    assert si.update_index(itype) == (30, 50)
    fresh = plain(d, m) if kind is None else refine(d, m, kind)
    fresh.set_codebooks(built.codebooks)
    fresh.add_with_ids(X2, ids2)
    want = tmp_path / "want.faiss"
    faiss_io.write_index(want, fresh.state_host())
    assert fn.read_bytes() == want.read_bytes()
    assert si.update_index(itype) == (0, 0)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement itself, and the recorded study
def test_restatement_is_the_list_scan_over_one_list_and_its_float32_trainer_follows_the_float64_one():
    rng = np.random.default_rng(2)
    N, d, m, nq, k = 700, 32, 4, 3, 20
    codes = rng.integers(0, 256, (N, m)).astype(np.uint8)
    codes[rng.random(N) < 0.2] = codes[0]
    lut = rng.standard_normal((nq, m, 256)).astype(np.float32)
    ids = rng.permutation(N).astype(np.int64) + 50
    D, I = ref.scan(codes, ids, lut, k)
    S = ref.scores(codes, lut)
    for q in range(nq):
        order = np.lexsort((np.arange(N), -S[q].astype(np.float64)))[:k]
        assert np.array_equal(D[q].view(np.uint32), S[q, order].view(np.uint32)) and np.array_equal(I[q], ids[order])
    Dp, Ip = ref.scan_pos(codes, ids, lut, np.arange(N), k)
    assert np.array_equal(Dp.view(np.uint32), D.view(np.uint32)) and np.array_equal(Ip, I)
    pos = np.arange(5, N, 7)
    Dp, Ip = ref.scan_pos(codes, None, lut, pos, k, id_base=9)
    D2, I2 = ref.scan(codes[pos], None, lut, k)
    assert np.array_equal(Dp.view(np.uint32), D2.view(np.uint32)) and np.array_equal(Ip, pos[I2] + 9)
    assert (ref.scan(codes[:0], None, lut, 3)[1] == -1).all()
    # the float32 trainer: the same codes as the float64 one off near ties, and a distortion within a rounding of its
    X = (rng.standard_normal((1500, d)) / np.sqrt(d)).astype(np.float32)
    cb32, cb64 = ref.train_f32(X, m, niter=3), ivfpq_ref.train(X, m, niter=3)
    assert cb32.dtype == np.float32 and np.array_equal(ref.train_f32(X, m, niter=0), ivfpq_ref.initial_codebooks(X, m))
    assert (ref.encode_f32(X, cb32) != ivfpq_ref.encode(X, cb32)).mean() < 1e-3
    a, b = ivfpq_ref.distortion(X, cb32), ivfpq_ref.distortion(X, cb64)
    assert abs(a - b) <= 1e-3 * b
    lut32 = ref.lut_f32(X[:4], cb32)
    assert lut32.dtype == np.float32 and np.abs(lut32 - ivfpq_ref.lut(X[:4], cb32)).max() < 1e-6
    dec = ref.decode(codes[:, :m], [0, -1, N, 5], cb32)
    assert np.isnan(dec[1:3]).all() and np.array_equal(dec[0], np.concatenate([cb32[j, codes[0, j]] for j in range(m)]))


def test_recall_study_on_one_more_seed(golden_dir):
    """The study of the issue as a seeded test: on the clustered study set (the bench tool's recipe, 60,000 x 128, m = 16, codebooks
    trained on the rows themselves, k = 10, 64 queries) re-ranking the 10 * 50 best PQ positions must lift recall@10 over the PQ scan
    alone by at least the smallest gain the restatement showed on five other seeds, less the spread of that gain
    (tests/golden/pq_flat_quality.json, written by `python tests/pq_flat_ref.py`).
    Recorded (five seeds): PQ alone 0.061 - 0.084; k_factor 50: R8 0.925 - 0.950, R16 0.966 - 0.972; k_factor 100 adds at most 0.007;
    k_factor 20: 0.56 - 0.62."""
    gold = json.loads((golden_dir / "pq_flat_quality.json").read_text())
    assert gold["seeds"] == [0, 1, 2, 3, 4] and len(gold["runs"]) == 5
    assert all(set(r["r8"]) == set(r["r16"]) == {"5", "10", "20", "50", "100"} for r in gold["runs"])
    assert {k: v for k, v in gold.items() if k.startswith("gain_")} == ref.study_summary(gold["runs"])
    r = ref.recall_study(5, dict(ref.STUDY, k_factors=(50,)))
    print(json.dumps(r))
    for kind in (8, 16):
        gain = r[f"r{kind}"]["50"] - r["pq_alone"]
        floor = gold[f"gain_min_r{kind}"] - gold[f"gain_spread_r{kind}"]
        print(f"R{kind}: gain {gain:.4f}, floor {floor:.4f}")
        assert floor > 0.3 and gain >= floor
    for run in gold["runs"] + [r]:                                       # PQ codes alone rank badly: the R forms are the useful ones
        assert run["pq_alone"] < 0.2 < run["r8"]["50"] <= run["r16"]["50"] + 0.01

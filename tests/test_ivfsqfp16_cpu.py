"""IndexIVFSQfp16 without a GPU: the float32 restatement (tests/ivfsqfp16_ref.py) against float64 and against the flat oracle, the
QT_fp16 flavour of the 'IwSq' file and its ranged reader, the index-type names, the recorded recall study, the entry points as the
header declares them, and the multi-rank build / load / collective search through the plugin surface at world size 2 over gloo
with a numpy stand-in for the index class (tests/test_gpu_ivfsqfp16*.py run the HIP kernels)."""
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

import ivfsqfp16_ref as h16
from wise_amd import _lib
from wise_amd.index import faiss_io

ROOT = Path(__file__).resolve().parent.parent
FID = "mlfoundations/open_clip/ViT-B-32/seeded-0"
ITYPE = "IndexIVFSQfp16"
NEW_SYMBOLS = {"wise_sq16_encode": 5, "wise_sq16_decode": 10, "wise_ivfsq16_scan": 17, "wise_ivfsq16_scan_sel": 18,
               "wise_ivfsq16_scan_local": 19, "wise_ivfsq16_range_count": 16, "wise_ivfsq16_range_fill": 18}


def unit_rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def small_index(N=700, d=48, nlist=9, seed=3):
    """(centroids, halves, ids, list_off) of N rows grouped into nlist lists (list 4 empty), with duplicated rows"""
    rng = np.random.default_rng(seed)
    c = unit_rows(nlist, d, seed + 1)
    X = unit_rows(N, d, seed + 2)
    X[N // 2:N // 2 + 40] = X[:40]
    a = (X @ c.T).argmax(axis=1)
    a[a == 4] = 5
    order = np.argsort(a, kind="stable")
    X, a = X[order], a[order]
    list_off = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=nlist))]).astype(np.int64)
    ids = rng.permutation(N).astype(np.int64) * 3 + 11
    return c, h16.encode((X - c[a]).astype(np.float32)), ids, list_off


def test_encoder_is_round_to_nearest_even_with_subnormals_and_overflow():
    f = np.float32
    x = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -15, -0.0, 0.0, 65504, 65519.99, 65520,
                  -1e9, 2.0 ** -14 - 2.0 ** -25], dtype=f)
    want = np.array([0x3C00, 0x3C02, 0x0001, 0x0000, 0x0002, 0x0200, 0x8000, 0x0000, 0x7BFF, 0x7BFF, 0x7C00, 0xFC00, 0x0400], dtype=np.uint16)
    assert np.array_equal(h16.encode(x[None, :]).view(np.uint16)[0], want)
    assert h16.decode(want.view(np.float16)[None, :]).dtype == np.float32


@pytest.mark.parametrize("d", [16, 48, 128, 512])
def test_restatement_is_within_the_summation_bound_of_float64(d):
    """score (float32, the scan's order) against float64 bias + q . h over the decoded halves: |delta| <= gamma_{d+2}
    (|bias| + sum |q_i h_i|), gamma_n = n 2^-24 / (1 - n 2^-24) — the bound for a sum of d + 2 float32 terms.  Derived, not measured."""
    c, halves, ids, list_off = small_index(N=600, d=d, seed=d)
    Q = unit_rows(5, d, d + 7) * np.float32(1.7)
    bias = (Q.astype(np.float64) @ c.astype(np.float64).T).astype(np.float32)
    lists = h16.list_of_rows(list_off)
    h64 = h16.decode(halves, np.float64)
    u = (d + 2) * 2.0 ** -24
    gamma = u / (1 - u)
    worst = 0.0
    for q in range(len(Q)):
        s = bias[q, lists] + h16.row_sums(halves, Q[q])
        assert s.dtype == np.float32
        ref = bias[q, lists].astype(np.float64) + h64 @ Q[q].astype(np.float64)
        bound = gamma * (np.abs(bias[q, lists]).astype(np.float64) + np.abs(h64 * Q[q].astype(np.float64)[None, :]).sum(axis=1))
        delta = np.abs(s.astype(np.float64) - ref)
        worst = max(worst, float((delta / bound).max()))
        assert (delta <= bound).all(), (d, q, float((delta / bound).max()))
    print(f"d={d}: largest |delta| / bound = {worst:.4f}")


def test_chunks_are_the_pieces_c_and_c_plus_C():
    d = 48
    e = h16.chunks(np.arange(d, dtype=np.float32)[None, :])[0]
    assert e.shape == (3, 16)
    assert e[1].tolist() == list(range(8, 16)) + list(range(32, 40))
    assert sorted(e.reshape(-1).tolist()) == list(range(d))


@pytest.mark.parametrize("d", [16, 48])
def test_lossless_case_equals_the_flat_oracle(d):
    """Rows and centroids on a dyadic grid: every residual is an exact half and every product and sum below is exact in float32, so
    with every list probed the restatement answers what the flat search over the fp32 rows answers."""
    from oracle import ip_topk_ref

    rng = np.random.default_rng(d)
    N, nlist, nq = 500, 7, 4
    c = rng.integers(-8, 9, (nlist, d)).astype(np.float32) / 8
    a = np.sort(rng.integers(0, nlist, N))
    X = c[a] + rng.integers(-32, 33, (N, d)).astype(np.float32) / 64
    X[N - 1] = X[0]                                              # a tie across two lists
    X[1] = X[0]                                                  # and inside one
    list_off = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=nlist))]).astype(np.int64)
    resid = X - c[a]
    halves = h16.encode(resid)
    assert np.array_equal(halves.astype(np.float32), resid)     # lossless
    Q = rng.integers(-16, 17, (nq, d)).astype(np.float32) / 16
    bias = (Q @ c.T).astype(np.float32)
    probes = np.tile(np.arange(nlist, dtype=np.int64), (nq, 1))
    for k in (1, 10, 64):
        D, I = h16.scan(halves, list_off, None, Q, probes, bias, k)
        Dr, Ir = ip_topk_ref.ip_topk(X, Q, k)
        assert np.array_equal(I, Ir), k
        assert np.abs(D.astype(np.float64) - Dr.astype(np.float64)).max() <= 2e-5


def test_scan_padding_skipped_probes_keep_and_ties():
    c, halves, ids, list_off = small_index(N=700, d=48, seed=58)
    nlist, N = len(c), len(halves)
    Q = unit_rows(4, 48, 99)
    bias = (Q.astype(np.float64) @ c.astype(np.float64).T).astype(np.float32)
    probes = np.tile(np.arange(nlist, dtype=np.int64), (len(Q), 1))
    D, I = h16.scan(halves, list_off, None, Q, probes, bias, N + 5)
    assert (I[:, N:] == -1).all() and (D[:, N:] == h16.NEG).all() and (I[:, :N] >= 0).all()
    for q in range(len(Q)):
        same = np.flatnonzero(D[q, 1:N].view(np.uint32) == D[q, :N - 1].view(np.uint32))
        assert len(same) > 0 and (I[q, same] < I[q, same + 1]).all()
    probes2 = probes.copy()
    probes2[:, 0] = -1
    probes2[:, 4] = nlist + 3                                    # (list 4 is empty anyway)
    D2, I2 = h16.scan(halves, list_off, ids, Q, probes2, bias, 10)
    keep = np.ones(N, bool)
    keep[list_off[0]:list_off[1]] = False
    D3, I3 = h16.scan(halves, list_off, ids, Q, probes, bias, 10, keep=keep)
    assert np.array_equal(I2, I3) and np.array_equal(D2.view(np.uint32), D3.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# the file
def _at_sq_record(c):
    return 4 + 33 + 16 + 4 + 33 + 8 + 4 * c.size + 9


def test_file_round_trip_and_the_two_flavours_of_the_record(tmp_path):
    c, halves, ids, list_off = small_index(N=500, d=16, nlist=9)
    fn = tmp_path / "video-IndexIVFSQfp16.faiss"
    state = {"centroids": c, "halves": halves, "ids": ids, "list_off": list_off}
    faiss_io.write_index(fn, state, nprobe=17)
    assert faiss_io.index_fourcc(fn) == "IwSq" and faiss_io.index_ntotal(fn) == 500
    f = faiss_io.read_index(fn)
    assert set(f) == {"centroids", "halves", "ids", "list_off", "nprobe"}           # no 'trained', no 'codes'
    assert f["halves"].dtype == np.float16 and f["halves"].tobytes() == halves.tobytes()
    assert np.array_equal(f["centroids"], c) and np.array_equal(f["ids"], ids) and np.array_equal(f["list_off"], list_off) and f["nprobe"] == 17
    raw = fn.read_bytes()
    at = _at_sq_record(c)
    assert struct.unpack_from("<iifQQQ", raw, at) == (4, 0, 0.0, 16, 32, 0)          # QT_fp16, code_size 2 d, nothing trained
    assert struct.unpack_from("<QB", raw, at + 36) == (32, 1)
    assert struct.unpack_from("<IQQ", raw, at + 45) == (faiss_io._fourcc("ilar"), 9, 32)
    first = int(np.flatnonzero(np.diff(list_off))[0])
    data = at + 45 + 20 + 12 + 8 * 9
    assert raw[data:data + 32] == halves[list_off[first]].astype("<f2").tobytes()      # the halves little-endian
    # written again from what was read: the same bytes
    faiss_io.write_index(tmp_path / "again.faiss", f)
    assert (tmp_path / "again.faiss").read_bytes() == raw
    # the family of the state and of the other flavour's
    from wise_amd.index import feature_search_index as fsi
    assert fsi._family_of_state(f) is fsi._family(ITYPE)
    fn8 = tmp_path / "video-IndexIVFSQ8.faiss"
    codes = np.random.default_rng(0).integers(0, 256, (500, 16), dtype=np.uint8)
    faiss_io.write_ivf_sq_ip(fn8, c, np.ones(32, np.float32), codes, ids, list_off)
    f8 = faiss_io.read_index(fn8)
    assert "halves" not in f8 and "trained" in f8 and f8["codes"].dtype == np.uint8
    assert fsi._family_of_state(f8) is fsi._family("IndexIVFSQ8") is not fsi._family(ITYPE)
    # a QT_fp16 file whose qtype field says QT_8bit (and the reverse) is refused, not read as the other flavour
    for src, q in ((raw, 0), (fn8.read_bytes(), 4)):
        bad = bytearray(src)
        struct.pack_into("<i", bad, at, q)
        (tmp_path / "bad.faiss").write_bytes(bytes(bad))
        with pytest.raises(RuntimeError, match="unsupported IndexIVFScalarQuantizer"):
            faiss_io.read_index(tmp_path / "bad.faiss")
    # any other quantizer type is still refused, and the message names both that are read
    for q in (1, 2, 3, 5, 6):
        bad = bytearray(raw)
        struct.pack_into("<i", bad, at, q)
        (tmp_path / "bad.faiss").write_bytes(bytes(bad))
        with pytest.raises(RuntimeError, match=rf"qtype={q}.*QT_8bit with one range per dimension is what is read.*QT_fp16"):
            faiss_io.read_index(tmp_path / "bad.faiss")
    # a file cut short is refused wherever the cut falls: in the lists, in the ids, in the record, in the header
    for cut in (len(raw) - 1, len(raw) - 8 * 500 - 3, at + 40, 20):
        (tmp_path / "cut.faiss").write_bytes(raw[:cut])
        with pytest.raises(RuntimeError):
            faiss_io.read_index(tmp_path / "cut.faiss")
    for reader in (faiss_io.read_ivf_flat_ip, faiss_io.read_ivf_pq_ip, faiss_io.read_idmap_flat_ip):
        with pytest.raises(RuntimeError):
            reader(fn)


@pytest.mark.parametrize("sizes", [
    [5, 0, 0, 17, 1, 0, 9, 0, 0, 0, 3, 12],           # most lists empty ('sprs' layout), lists straddle boundaries
    [40, 3, 8, 2, 11, 6, 1, 4, 9, 2],                 # 'full' layout, one list larger than a rank's share
    [0, 0, 0],                                        # no rows at all
])
def test_range_reader_equals_slices_of_the_whole_reader(tmp_path, sizes):
    from wise_amd.index.sharded import shard_range

    d = 16
    rng = np.random.default_rng(len(sizes))
    sizes = np.asarray(sizes, dtype=np.int64)
    n = int(sizes.sum())
    w = {"centroids": rng.standard_normal((len(sizes), d)).astype(np.float32),
         "halves": rng.integers(0, 0x7C00, (n, d)).astype(np.uint16).view(np.float16),   # any finite bit pattern
         "ids": rng.permutation(10 * n + 1)[:n].astype(np.int64) + 3,
         "list_off": np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)}
    fn = tmp_path / "x.faiss"
    faiss_io.write_index(fn, w, nprobe=7)
    full = faiss_io.read_index(fn)
    assert full["halves"].tobytes() == w["halves"].tobytes() and faiss_io.index_ntotal(fn) == n
    for W in (1, 2, 5):
        parts = []
        for r in range(W):
            lo, hi = shard_range(n, r, W)
            p = faiss_io.read_index_range(fn, lo, hi)
            assert set(p) == set(full) and p["nprobe"] == 7 and np.array_equal(p["centroids"], w["centroids"])
            assert p["halves"].dtype == np.float16 and p["halves"].tobytes() == full["halves"][lo:hi].tobytes()
            assert np.array_equal(p["ids"], full["ids"][lo:hi])
            assert np.array_equal(p["list_off"], np.clip(full["list_off"] - lo, 0, hi - lo)), (W, r)
            parts.append(p)
        assert np.array_equal(sum(p["list_off"] for p in parts), full["list_off"]), W
    if n:
        short = tmp_path / "short.faiss"
        short.write_bytes(fn.read_bytes()[:-12])
        with pytest.raises(RuntimeError, match="cut short"):
            faiss_io.read_index_range(short, n - 1, n)


# ---------------------------------------------------------------------------------------------------------------------
# names
def _store(tmp_path, d, n=12):
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    from wise_amd.index.search_index_factory import SearchIndexFactory

    fdir, idir = tmp_path / "features", tmp_path / "index"
    fdir.mkdir(parents=True)
    X = unit_rows(n, d, 9)
    st = FeatureStoreFactory.create_store(FeatureStoreType.WEBDATASET, "video", str(fdir))
    st.enable_write(2048, 20 * 1024 * 1024)
    for i in range(n):
        st.add(i + 1, X[i:i + 1])
    st.close()
    return SearchIndexFactory("video", "mlfoundations/open_clip/ViT-B-32/seeded-0", {"features_dir": fdir, "index_dir": idir})


def test_create_index_names(tmp_path, monkeypatch):
    from wise_amd.index import feature_search_index as fsi

    si = _store(tmp_path, 64)
    for bad in ("IndexIVFSQ4", "IndexIVFSQ", "IndexIVFSQfp32"):
        with pytest.raises(NotImplementedError, match="IndexFlatIP, IndexIVFFlat and IndexIVFPQ<m>.*IndexIVFSQfp16"):
            si.create_index(bad)
        with pytest.raises(NotImplementedError):
            si.update_index(bad)
        assert not si.get_index_filename(bad).exists()
    assert si.get_index_filename(ITYPE).name == "video-IndexIVFSQfp16.faiss"
    fam = fsi._family(ITYPE)
    assert fam.trained == () and fam.payload == "halves" and fam.marks == {"halves"} and fam.factory == "ivfsqfp16_index_factory"
    assert issubclass(fam.wrapper, fsi.ShardedIVFSQIPIndex) and fam.cls() is fsi.IVFSQfp16IPIndex
    assert fsi.FeatureSearchIndex.ivfsqfp16_index_factory is fsi.IVFSQfp16IPIndex and issubclass(fsi.IVFSQfp16IPIndex, fsi.IVFSQIPIndex)

    class Accepted(Exception):
        pass

    class StandIn:                                                # the name reaches the index class: no GPU here
        def __init__(self, d, nlist):
            raise Accepted(f"{d} {nlist}")

    monkeypatch.setattr(fsi, "IVFSQfp16IPIndex", StandIn)
    with pytest.raises(Accepted, match="64 "):
        si.create_index(ITYPE)
    si40 = _store(tmp_path / "b", 40)
    with pytest.raises(ValueError, match="multiple of 16"):
        si40.create_index(ITYPE)                                  # refused before a row is read


def test_header_declares_and_library_exports_the_entry_points():
    from wise_amd.build import declared_symbols

    declared = set(declared_symbols())
    assert set(_lib.SIGNATURES) == declared
    lib = _lib.load()
    header = (ROOT / "include" / "wise_hip.h").read_text()
    for name, nargs in NEW_SYMBOLS.items():
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
        decl = re.search(r"\bint\s+" + name + r"\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]) == nargs, name
    assert lib.wise_abi_version() == 5
    assert not [n for n in declared if "sq16" in n and "workspace" in n]              # the SQ8 workspace sizes serve both
    from wise_amd.index import IVFSQfp16IPIndex
    from wise_amd.index.ivf_sq import IVFSQfp16IPIndex as direct
    assert IVFSQfp16IPIndex is direct


def test_recorded_recall_study_first_seed_and_the_gap_to_ivfflat():
    gold = json.loads((ROOT / "tests" / "golden" / "ivfsqfp16_quality.json").read_text())
    gold8 = json.loads((ROOT / "tests" / "golden" / "ivfsq_quality.json").read_text())
    assert gold["seeds"] == [0, 1, 2, 3, 4] and json.dumps(h16.STUDY) in gold["what"] and json.dumps(h16.STUDY) in gold8["what"]
    run = h16.recall_study(gold["seeds"][0])
    assert run == gold["runs"][0], (run, gold["runs"][0])
    assert gold["sqfp16_min"] == min(r["sqfp16"] for r in gold["runs"])
    assert gold["gap_max"] == max(r["ivfflat"] - r["sqfp16"] for r in gold["runs"])
    assert [r["ivfflat"] for r in gold["runs"]] == [r["ivfflat"] for r in gold8["runs"]]       # the same sets
    assert gold["gap_max"] < gold8["gap_max"]                    # the 16-bit point sits closer to IVFFlat than the 8-bit one


# ---------------------------------------------------------------------------------------------------------------------
# the plugin surface at world size 2 (gloo) with a numpy stand-in for IVFSQfp16IPIndex
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


class _DirectMap:
    def __init__(self):
        self.type = 0


class _CpuIVFSQfp16:
    """What FeatureSearchIndex.ivfsqfp16_index_factory must offer: train / centroids / set_centroids / encode_rows /
    adopt_lists(pos_base) / nprobe / search_local_device / reconstruct_batch / lists_host (and merge_lists for the wrapper)."""

    def __init__(self, d, nlist):
        self.d, self.nlist, self.device = int(d), int(nlist), torch.device("cpu")
        self.nprobe, self.parallel_mode, self.direct_map = 1, 0, _DirectMap()
        self.centroids = None
        self.halves, self.ids, self.list_off, self.pos_base = np.zeros((0, d), np.float16), np.zeros(0, np.int64), np.zeros(nlist + 1, np.int64), 0

    @property
    def is_trained(self):
        return self.centroids is not None

    def train(self, x):
        c = np.asarray(x, np.float64)[:self.nlist]                    # deterministic stand-in for k-means
        self.set_centroids((c / np.linalg.norm(c, axis=1, keepdims=True)).astype(np.float32))

    def set_centroids(self, c):
        self.centroids = np.array(c, dtype=np.float32)

    def _assign(self, x):
        return (np.asarray(x, np.float64) @ self.centroids.astype(np.float64).T).argmax(axis=1).astype(np.int64)

    def encode_rows(self, x):
        x = np.asarray(x, np.float32)
        a = self._assign(x)
        return a, h16.encode(x - self.centroids[a])

    def add_with_ids(self, x, ids):
        a, halves = self.encode_rows(x)
        order = np.argsort(a, kind="stable")
        off = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=self.nlist))]).astype(np.int64)
        self.adopt_lists(torch.from_numpy(halves[order]), torch.from_numpy(np.asarray(ids, np.int64)[order]), torch.from_numpy(off))

    def adopt_lists(self, halves, ids, list_off, pos_base=0):
        assert halves.dtype == torch.float16
        self.halves, self.ids, self.list_off, self.pos_base = halves.numpy().copy(), ids.numpy().copy(), list_off.numpy().copy(), int(pos_base)
        return self

    def lists_host(self):
        return self.centroids, self.halves, self.ids, self.list_off

    @property
    def ntotal(self):
        return self.halves.shape[0]

    def hbm_bytes(self):
        return self.halves.nbytes + self.ids.nbytes

    def make_direct_map(self, enable=True):
        self.direct_map.type = 2 if enable else 0

    def search_local_device(self, q, k, probe_count=None, positions=False):
        from oracle import ivf_ref

        Q = q.numpy()
        probes = ivf_ref.coarse_probes(self.centroids, Q, min(self.nprobe, self.nlist))
        coarse = Q.astype(np.float64) @ self.centroids.astype(np.float64).T
        bias = np.take_along_axis(coarse, probes, axis=1).astype(np.float32)
        D, I = h16.scan(self.halves, self.list_off, None if positions else self.ids, Q, probes, bias, k)
        return torch.from_numpy(D), torch.from_numpy(np.where(I >= 0, I + self.pos_base, -1) if positions else I)

    search_device = search_local_device

    def reconstruct_batch(self, want):
        out = np.full((len(want), self.d), np.nan, np.float32)
        rows = h16.decode_rows(self.halves, self.list_off, self.centroids)
        for i, w in enumerate(want):
            hit = np.flatnonzero(self.ids == w)
            if len(hit):
                out[i] = rows[hit[0]]
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


WANT_IDS = [1, 1001, 500, 1006]


def _plugin_worker(rank, world, port, root, N, d):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["WISE_SHARDED_IVF"] = "1"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import wise_amd.index.feature_search_index as fsi
    from wise_amd.index.search_index_factory import SearchIndexFactory
    from wise_amd.index.selector import IDSelectorRange, SearchParameters
    from wise_amd.index.sharded import NO_SELECTOR, ShardedIVFSQfp16IPIndex, shard_range

    fsi.FeatureSearchIndex.ivfsqfp16_index_factory = _CpuIVFSQfp16
    fsi.FeatureExtractorFactory = lambda fid: _FakeTextTower(d)
    root = Path(root)
    Q = np.random.default_rng(6).standard_normal((3, d)).astype(np.float32)
    out = {}
    # (A) the collective build: own store shards -> one part file per rank -> load the part
    si = SearchIndexFactory("video", FID, {"features_dir": root / "features", "index_dir": root / "index_parts"})
    si.create_index(ITYPE)
    part = si.get_index_part_filename(ITYPE, rank, world)
    assert part.exists() and not si.get_index_filename(ITYPE).exists() and faiss_io.index_fourcc(part) == "IwSq"
    dist.barrier()
    # (B) rank 0 lays the parts end to end into one file; (A) loads the parts, (B) every rank its range of that file
    sdir = root / "index_single"
    if rank == 0:
        ps = [faiss_io.read_index(si.get_index_part_filename(ITYPE, r, world)) for r in range(world)]
        sdir.mkdir()
        faiss_io.write_index(sdir / si.get_index_filename(ITYPE).name,
                             {"centroids": ps[0]["centroids"], "halves": np.concatenate([p["halves"] for p in ps]),
                              "ids": np.concatenate([p["ids"] for p in ps]), "list_off": sum(p["list_off"] for p in ps)}, nprobe=8)
    dist.barrier()
    for tag, idir in (("A", root / "index_parts"), ("B", sdir)):
        s = SearchIndexFactory("video", FID, {"features_dir": root / "features", "index_dir": idir})
        assert s.load_index(ITYPE) is True
        idx = s.index
        assert type(idx) is ShardedIVFSQfp16IPIndex and idx.is_trained and idx.local.pos_base == shard_range(N, rank, world)[0]
        idx.nprobe = 8
        assert idx.hbm_bytes() == idx.local.hbm_bytes()
        with pytest.raises(NotImplementedError) as e:
            idx.search(Q, 3, params=SearchParameters(sel=IDSelectorRange(0, 10)))
        assert str(e.value) == NO_SELECTOR
        with pytest.raises(NotImplementedError):
            idx.range_search(Q, 0.1)
        with pytest.raises(NotImplementedError):
            idx.remove_ids(np.array([1]))
        out[f"{tag}_dist"], out[f"{tag}_ids"] = s.search("video", "dog", topk=7)
        out[f"{tag}_D"], out[f"{tag}_I"] = idx.search(Q, 25)
        out[f"{tag}_rec"] = idx.reconstruct_batch(np.array(WANT_IDS, dtype=np.int64))
        out[f"{tag}_ntotal"] = np.array([idx.ntotal])
        out[f"{tag}_xbytes"] = np.array([idx.last_exchange_bytes])
    np.savez(root / f"ivfsqfp16_rank{rank}.npz", **out)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_through_the_plugin_surface_world2(tmp_path):
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    from wise_amd.index.ivf_flat import reference_nlist
    from wise_amd.index.sharded import shard_range

    N, d, world = 1001, 32, 2
    X = np.random.default_rng(5).standard_normal((N, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X[700] = X[20]                                                       # equal rows on both ranks' slices
    fdir = tmp_path / "features"
    fdir.mkdir()
    st = FeatureStoreFactory.create_store(FeatureStoreType.WEBDATASET, "video", str(fdir))
    st.enable_write(100, 20 * 1024 * 1024)                               # 11 tar files: ranks get 6 and 5 of them
    for i in range(N):
        st.add(i + 1, X[i:i + 1])
    st.close()
    mp.spawn(_plugin_worker, args=(world, _free_port(), str(tmp_path), N, d), nprocs=world, join=True)

    # what every rank read from the store, in rank order: the sharded build's source order
    rows, rids = [], []
    for r in range(world):
        rd = FeatureStoreFactory.load_store("video", fdir)
        rd.enable_read(shard_shuffle=False, shard_slice=(r, world))
        for fids, vecs in rd.iter_batch():
            rows.append(np.asarray(vecs, np.float32))
            rids.append(np.asarray(fids, np.int64))
    Xcat, idcat = np.concatenate(rows), np.concatenate(rids)
    nlist = reference_nlist(N)
    sample = np.sort(np.random.default_rng(1234).permutation(N)[:min(N, 100 * nlist)])
    ref = _CpuIVFSQfp16(d, nlist)
    ref.train(Xcat[sample])
    ref.add_with_ids(Xcat, idcat)                                        # one process over the same rows in the same order
    one = tmp_path / "one-process.faiss"
    faiss_io.write_index(one, dict(zip(("centroids", "halves", "ids", "list_off"), ref.lists_host())), nprobe=8)
    # the part files laid end to end (what rank 0 wrote in (B)) are that file, byte for byte
    assert (tmp_path / "index_single" / f"video-{ITYPE}.faiss").read_bytes() == one.read_bytes()
    for r in range(world):
        p = faiss_io.read_index(tmp_path / "index_parts" / f"video-{ITYPE}.faiss.part-{r:03d}-of-{world:03d}")
        lo, hi = shard_range(N, r, world)
        assert p["halves"].tobytes() == ref.halves[lo:hi].tobytes() and np.array_equal(p["ids"], ref.ids[lo:hi]), r
        assert np.array_equal(p["list_off"], np.clip(ref.list_off - lo, 0, hi - lo)), r
    # the whole stand-in answers what the collective search answers
    ref.nprobe = 8
    q1 = torch.from_numpy(_FakeTextTower(d).extract_text_features(["This is a photo of a dog"]))
    Q = torch.from_numpy(np.random.default_rng(6).standard_normal((3, d)).astype(np.float32))
    D1, I1 = (t.numpy() for t in ref.search_device(q1, 7))
    D3, I3 = (t.numpy() for t in ref.search_device(Q, 25))
    assert (I3 >= 0).all() and (I1 >= 0).all()
    rec_ref = ref.reconstruct_batch(WANT_IDS)
    assert np.isfinite(rec_ref[:3]).all() and np.isnan(rec_ref[3]).all()
    for r in range(world):
        g = np.load(tmp_path / f"ivfsqfp16_rank{r}.npz")
        for tag in "AB":
            assert np.array_equal(g[f"{tag}_ids"], I1[0]) and np.array_equal(g[f"{tag}_dist"], D1[0]), (r, tag)
            assert np.array_equal(g[f"{tag}_I"], I3) and np.array_equal(g[f"{tag}_D"], D3), (r, tag)
            assert np.array_equal(g[f"{tag}_rec"], rec_ref, equal_nan=True), (r, tag)
            assert int(g[f"{tag}_ntotal"][0]) == N
            assert int(g[f"{tag}_xbytes"][0]) == 16 * 3 * 25, (r, tag)

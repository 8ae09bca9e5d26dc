"""IndexIVFOPQ without a GPU: the index-type names, the 'WiOP' file (round trip, ranged readers, refusals), the float64
restatement of the trainer (tests/ivfopq_ref.py) and what tests/golden/ivfopq_quality.json records of it, and the C ABI's new
entry points as the header declares and the library exports them."""
import json
import re
import struct
from pathlib import Path

import numpy as np
import pytest

import ivfopq_ref
import ivfpq_ref
import ivfpq_refine_ref as rr
from wise_amd.index import faiss_io
from wise_amd.index.feature_search_index import (parse_ivfopq_refine_type, parse_ivfopq_type, parse_ivfpq_refine_type,
                                                 parse_ivfpq_type)

ROOT = Path(__file__).resolve().parent.parent


def unit_rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


# --------------------------------------------------------------------------------------------------------------------- names
def test_index_type_names():
    assert parse_ivfopq_type("IndexIVFOPQ64", 512) == 64
    assert parse_ivfopq_type("IndexIVFOPQ", 512) == 128
    assert parse_ivfopq_type("IndexIVFOPQ96", 768) == 96
    assert parse_ivfopq_type("IndexIVFOPQ") == 0
    assert parse_ivfopq_refine_type("IndexIVFOPQ64R8", 512) == (64, 8)
    assert parse_ivfopq_refine_type("IndexIVFOPQ16R16", 512) == (16, 16)
    assert parse_ivfopq_refine_type("IndexIVFOPQR16", 512) == (128, 16)
    with pytest.raises(ValueError, match=r"m <= 128.*IndexIVFOPQ<m>"):
        parse_ivfopq_type("IndexIVFOPQ", 768)                    # the bare name: m = d / 4 = 192
    with pytest.raises(ValueError, match="not a multiple of m"):
        parse_ivfopq_type("IndexIVFOPQ7", 512)
    with pytest.raises(ValueError, match=r"out of \[1, 128\]"):
        parse_ivfopq_type("IndexIVFOPQ192", 768)
    with pytest.raises(ValueError, match="re-ranking stores are R8"):
        parse_ivfopq_refine_type("IndexIVFOPQ64R4", 512)
    with pytest.raises(ValueError, match=r"multiple of 4 in \[4, 1024\]"):
        parse_ivfopq_type("IndexIVFOPQ64", 2048)                 # the rotation's own limit
    # neither family reads the other's names, and nothing else is read at all
    for other in ("IndexFlatIP", "IndexIVFFlat", "IndexHNSWFlat", "IndexIVFOPQx", "IndexIVFOPQ-4", "IndexIVFPQ64", "IndexIVFPQ64R8",
                  "IndexOPQ64"):
        assert parse_ivfopq_type(other, 512) is None and parse_ivfopq_refine_type(other, 512) is None
    for name in ("IndexIVFOPQ64", "IndexIVFOPQ64R8", "IndexIVFOPQ"):
        assert parse_ivfpq_type(name, 512) is None and parse_ivfpq_refine_type(name, 512) is None
    # the IndexIVFPQ names parse exactly as before
    assert parse_ivfpq_type("IndexIVFPQ64", 512) == 64 and parse_ivfpq_type("IndexIVFPQ", 512) == 128 and parse_ivfpq_type("IndexIVFPQ") == 0
    assert parse_ivfpq_refine_type("IndexIVFPQ64R8", 512) == (64, 8) and parse_ivfpq_type("IndexIVFPQ64R8", 512) is None
    with pytest.raises(ValueError, match=r"m <= 128.*IndexIVFPQ<m>"):
        parse_ivfpq_type("IndexIVFPQ", 768)
    assert parse_ivfpq_type("IndexIVFPQ64", 2048) == 64          # no rotation, no d <= 1024 rule


def _store(tmp_path, d, n=12):
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    from wise_amd.index.search_index_factory import SearchIndexFactory

    fdir, idir = tmp_path / "features", tmp_path / "index"
    fdir.mkdir()
    X = unit_rows(n, d, 9)
    st = FeatureStoreFactory.create_store(FeatureStoreType.WEBDATASET, "video", str(fdir))
    st.enable_write(2048, 20 * 1024 * 1024)
    for i in range(n):
        st.add(i + 1, X[i:i + 1])
    st.close()
    return SearchIndexFactory("video", "mlfoundations/open_clip/ViT-B-32/seeded-0", {"features_dir": fdir, "index_dir": idir})


def test_create_index_refuses_bad_names_before_any_gpu_work(tmp_path):
    si = _store(tmp_path, 768)
    with pytest.raises(NotImplementedError, match="IndexFlatIP, IndexIVFFlat and IndexIVFPQ<m>"):
        si.create_index("IndexOPQ64")
    with pytest.raises(NotImplementedError):
        si.create_index("IndexIVFOPQx")
    with pytest.raises(ValueError, match="IndexIVFOPQ<m>"):
        si.create_index("IndexIVFOPQ")                           # m = d / 4 = 192 at d = 768
    with pytest.raises(ValueError):
        si.create_index("IndexIVFOPQ7")
    with pytest.raises(ValueError, match="R8"):
        si.create_index("IndexIVFOPQ64R4")
    assert si.get_index_filename("IndexIVFOPQ64R8").name == "video-IndexIVFOPQ64R8.faiss"
    assert not si.get_index_filename("IndexIVFOPQ").exists()


# --------------------------------------------------------------------------------------------------------------------- file
def _opq_file(path, sizes, d, m, seed, kind=None):
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    n = int(sizes.sum())
    f = {"list_off": np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
         "codes": rng.integers(0, 256, size=(n, m), dtype=np.uint8),
         "ids": rng.permutation(10 * n + 1)[:n].astype(np.int64) + 3,
         "centroids": rng.standard_normal((len(sizes), d)).astype(np.float32),
         "codebooks": rng.standard_normal((m, 256, d // m)).astype(np.float32),
         "rotation": ivfopq_ref.procrustes(rng.standard_normal((d, d))).astype(np.float32)}
    head = (f["rotation"], f["centroids"], f["codebooks"], f["codes"], f["ids"], f["list_off"])
    if kind is None:
        faiss_io.write_ivf_opq_ip(path, *head, nprobe=7)
    else:
        f["rows"], f["scales"] = rr.quantise(rng.standard_normal((n, d)).astype(np.float32), kind)
        faiss_io.write_ivf_opq_ip(path, *head, nprobe=7, kind=kind, k_factor=20, rows=f["rows"], scales=f["scales"])
    return f


@pytest.mark.parametrize("kind", [None, 8, 16])
def test_wiop_file_round_trip(tmp_path, kind):
    fn = tmp_path / "video-IndexIVFOPQ4.faiss"
    d, m = 16, 4
    w = _opq_file(fn, [40, 3, 0, 2, 11, 6, 1, 4, 9], d, m, seed=3, kind=kind)
    assert faiss_io.index_fourcc(fn) == "WiOP"
    f = faiss_io.read_ivf_opq_ip(fn)
    for a in ("rotation", "centroids", "codebooks", "codes", "ids", "list_off"):
        assert f[a].dtype == w[a].dtype and np.array_equal(f[a], w[a]), a
    assert f["nprobe"] == 7 and faiss_io.ivf_opq_ip_ntotal(fn) == 76 and ("kind" in f) == (kind is not None)
    if kind is not None:
        assert f["kind"] == kind and f["k_factor"] == 20 and np.array_equal(f["rows"], w["rows"])
        assert f["scales"] is None if kind == 16 else np.array_equal(f["scales"], w["scales"])
    # the layout: fourcc, version, d, R row-major, then a complete record of the wrapped kind — readable on its own
    raw = fn.read_bytes()
    assert struct.unpack_from("<III", raw, 0) == (faiss_io._fourcc("WiOP"), 1, d)
    assert np.array_equal(np.frombuffer(raw, np.float32, d * d, 12).reshape(d, d), w["rotation"])
    inner = tmp_path / "inner.faiss"
    inner.write_bytes(raw[12 + 4 * d * d:])
    assert faiss_io.index_fourcc(inner) == ("IwPQ" if kind is None else "WiPR")
    g = (faiss_io.read_ivf_pq_ip if kind is None else faiss_io.read_ivf_pq_refine_ip)(inner)
    assert np.array_equal(g["codes"], w["codes"]) and np.array_equal(g["ids"], w["ids"])
    # the other readers refuse it, and it refuses the other files
    for other in (faiss_io.read_ivf_pq_ip, faiss_io.read_ivf_pq_refine_ip, faiss_io.read_ivf_flat_ip, faiss_io.read_idmap_flat_ip):
        with pytest.raises(RuntimeError):
            other(fn)
    for reader in (faiss_io.read_ivf_opq_ip, faiss_io.ivf_opq_ip_ntotal, lambda p: faiss_io.read_ivf_opq_ip_range(p, 0, 1)):
        with pytest.raises(RuntimeError, match="not an IndexIVFOPQ file"):
            reader(inner)
    with pytest.raises(RuntimeError, match="No such file"):
        faiss_io.read_ivf_opq_ip(tmp_path / "absent.faiss")


def test_wiop_wrong_version_or_d_is_refused(tmp_path):
    fn = tmp_path / "x.faiss"
    d, m = 16, 4
    _opq_file(fn, [5, 7, 3], d, m, seed=1)
    raw = fn.read_bytes()
    bad = tmp_path / "bad.faiss"
    bad.write_bytes(raw[:4] + struct.pack("<I", 2) + raw[8:])                              # a version this reader does not know
    with pytest.raises(RuntimeError, match="version 2"):
        faiss_io.read_ivf_opq_ip(bad)
    with pytest.raises(RuntimeError, match="version 2"):
        faiss_io.ivf_opq_ip_ntotal(bad)
    bad.write_bytes(raw[:8] + struct.pack("<I", 0) + raw[12:])                             # d = 0
    with pytest.raises(RuntimeError, match="not an IndexIVFOPQ file"):
        faiss_io.read_ivf_opq_ip(bad)
    # a rotation of another d than the index behind it: a 4 x 4 matrix, then the record of d = 16
    bad.write_bytes(raw[:8] + struct.pack("<I", 4) + raw[12:12 + 4 * 16] + raw[12 + 4 * d * d:])
    with pytest.raises(RuntimeError, match="rotation of d = 4 in front of an index of d = 16"):
        faiss_io.read_ivf_opq_ip(bad)
    with pytest.raises(RuntimeError, match="rotation of d = 4"):
        faiss_io.read_ivf_opq_ip_range(bad, 0, 5)
    bad.write_bytes(raw[:12 + 4 * d * d] + b"IxFI" + raw[16 + 4 * d * d:])                 # wraps something else
    with pytest.raises(RuntimeError, match="wraps record type"):
        faiss_io.read_ivf_opq_ip(bad)
    bad.write_bytes(raw[:100])                                                             # cut short inside the rotation
    with pytest.raises(RuntimeError, match="cut short"):
        faiss_io.read_ivf_opq_ip(bad)
    with pytest.raises(AssertionError):
        faiss_io.write_ivf_opq_ip(bad, np.eye(8, dtype=np.float32), np.zeros((2, 16), np.float32), np.zeros((4, 256, 4), np.float32),
                                  np.zeros((0, 4), np.uint8), np.zeros(0, np.int64), np.zeros(3, np.int64))


@pytest.mark.parametrize("kind", [None, 8, 16])
@pytest.mark.parametrize("sizes", [
    [5, 0, 0, 17, 1, 0, 9, 0, 0, 0, 3, 12],           # most lists empty ('sprs' layout), lists straddle boundaries
    [40, 3, 8, 2, 11, 6, 1, 4, 9, 2],                 # 'full' layout, one list larger than a rank's share
    [0, 0, 0, 6, 0, 0],                               # one non-empty list: all ranks cut the same list
    [0, 0, 0],                                        # no rows at all
])
def test_range_readers_tile_the_file(tmp_path, sizes, kind):
    from wise_amd.index.sharded import shard_range

    fn = tmp_path / "x.faiss"
    d, m = 16, 4
    w = _opq_file(fn, sizes, d, m, seed=len(sizes), kind=kind)
    full = faiss_io.read_ivf_opq_ip(fn)
    n = w["codes"].shape[0]
    assert np.array_equal(full["codes"], w["codes"]) and np.array_equal(full["list_off"], w["list_off"]) and faiss_io.ivf_opq_ip_ntotal(fn) == n
    arrays = ["codes", "ids"] + ([] if kind is None else ["rows"]) + (["scales"] if kind == 8 else [])
    for W in (1, 2, 3, 8):
        parts = []
        for r in range(W):
            lo, hi = shard_range(n, r, W)
            p = faiss_io.read_ivf_opq_ip_range(fn, lo, hi)
            assert np.array_equal(p["rotation"], w["rotation"]) and np.array_equal(p["centroids"], w["centroids"])
            assert np.array_equal(p["codebooks"], w["codebooks"]) and p["nprobe"] == 7
            assert p["codes"].shape == (hi - lo, m) and p["ids"].shape == (hi - lo,)
            assert np.array_equal(p["list_off"], np.clip(w["list_off"] - lo, 0, hi - lo)), (W, r)
            if kind is not None:
                assert p["kind"] == kind and p["k_factor"] == 20 and p["rows"].shape == (hi - lo, d) and p["rows"].dtype == w["rows"].dtype
                assert (p["scales"] is None) == (kind == 16)
            parts.append(p)
        for a in arrays:
            assert np.array_equal(np.concatenate([p[a] for p in parts]), w[a]), (W, a)
        assert np.array_equal(sum(p["list_off"] for p in parts), full["list_off"]), W    # the clipped offsets add up
    with pytest.raises(ValueError):
        faiss_io.read_ivf_opq_ip_range(fn, 0, n + 1)


# --------------------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("d", [8, 64, 512])
def test_procrustes_is_orthonormal_and_optimal(d):
    rng = np.random.default_rng(d)
    M = rng.standard_normal((d, d))
    M[:, : d // 4] = 0.0                                          # rank-deficient: codewords that never use some directions
    R = ivfopq_ref.procrustes(M)
    assert np.abs(R @ R.T - np.eye(d)).max() <= d * 2.0 ** -50
    # R maximises trace(R M^T) over orthonormal matrices: no random rotation does better, and neither does the identity
    best = np.trace(R @ M.T)
    for _ in range(5):
        other = ivfopq_ref.procrustes(rng.standard_normal((d, d)))
        assert np.trace(other @ M.T) <= best
    assert np.trace(M) <= best


def test_rotation_recovers_a_known_mixing():
    """Residuals that ARE codewords of an axis-aligned quantizer, turned by a known orthogonal matrix: one Procrustes step from
    the true assignment undoes the turn, and the rotated residuals are then quantised without loss."""
    n, d, m = 4000, 16, 4
    rng = np.random.default_rng(2)
    cb = rng.standard_normal((m, 256, d // m))
    codes = rng.integers(0, 256, (n, m)).astype(np.uint8)
    y = ivfopq_ref.codewords(codes, cb)
    T = ivfopq_ref.procrustes(rng.standard_normal((d, d)))
    x = y @ T                                                     # x_i = T^T y_i, so R = T maps x back onto y
    R = ivfopq_ref.procrustes(ivfopq_ref.correlation(codes, cb, x))
    assert np.abs(R - T).max() < 1e-9
    assert abs(ivfopq_ref.distortion(x, R, cb)) < 1e-12 < 1e-3 < ivfopq_ref.distortion(x, np.eye(d), cb)
    assert np.array_equal(ivfopq_ref.encode(ivfopq_ref.rotate(x, R), cb), codes)
    assert np.array_equal(ivfopq_ref.encode(y, cb), ivfpq_ref.encode(y, cb))


def test_small_training_never_raises_the_distortion():
    X = ivfopq_ref.decaying_spectrum_rows(3000, 32, 12, 0.6, seed=5)
    c = ivfpq_ref.spherical_kmeans(X, 12, 1)
    _, resid = ivfopq_ref.residuals(X, c)
    R, cb, hist = ivfopq_ref.train(resid, 8, niter=3, opq_niter=6, opq_niter_pq=2)
    assert len(hist) == 7 and all(b <= a for a, b in zip(hist, hist[1:])) and hist[-1] < 0.9 * hist[0]
    assert np.abs(R @ R.T - np.eye(32)).max() <= 32 * 2.0 ** -50
    assert hist[0] == pytest.approx(ivfpq_ref.distortion(resid, ivfpq_ref.train(resid, 8, niter=3)), rel=1e-6)      # iteration 0 is plain PQ
    assert hist[-1] == pytest.approx(ivfopq_ref.distortion(resid, R, cb), rel=1e-12)


def test_golden_records_a_falling_distortion(golden_dir):
    gold = json.loads((golden_dir / "ivfopq_quality.json").read_text())
    hist = gold["distortion_per_iteration"]
    assert len(hist) == 51 and len(gold["distortion"]) == len(gold["seeds"]) == len(gold["recall_at_10"]) == 5
    assert all(b <= a for a, b in zip(hist, hist[1:]))            # never rises
    assert hist[-1] <= hist[0] and hist[-1] == gold["distortion"][0]
    dist = np.array(gold["distortion"])
    assert gold["distortion_margin"] == pytest.approx((dist.max() - dist.min()) / dist.min(), rel=1e-12)
    assert gold["recall_allowance"] == pytest.approx(max(gold["recall_at_10"]) - min(gold["recall_at_10"]), abs=1e-12)
    assert 0 < gold["distortion_margin"] < 0.1 and 0 <= gold["recall_allowance"] < 0.1
    # the golden's data is what ivfopq_ref.study_data() builds, and its first figure is plain PQ's on that data
    p = ivfopq_ref.STUDY
    assert json.loads(gold["what"].split(": ", 1)[1]) == p
    X, _, c = ivfopq_ref.study_data()
    _, resid = ivfopq_ref.residuals(X, c)
    rt = resid[ivfpq_ref.training_rows(p["n"], gold["seeds"][0])]
    e0 = ivfpq_ref.distortion(rt, ivfpq_ref.train(rt, p["m"], niter=10))
    assert e0 == pytest.approx(hist[0], rel=1e-6) and e0 == pytest.approx(gold["distortion_pq"], rel=1e-6)


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_header_declares_and_library_exports_the_opq_entry_points():
    from wise_amd import _lib
    from wise_amd.build import HIP_SOURCES, declared_symbols

    header = (ROOT / "include" / "wise_hip.h").read_text()
    names = ("wise_opq_rotate", "wise_opq_corr_workspace_bytes", "wise_opq_corr", "wise_opq_decode")
    for name in names:
        assert name in declared_symbols() and name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert "opq.hip" in HIP_SOURCES
    assert [len(_lib.SIGNATURES[n][1]) for n in names] == [6, 2, 10, 13]
    assert re.search(r"added within 5:.*wise_opq_rotate,\s+\* wise_opq_corr \(with wise_opq_corr_workspace_bytes\) and wise_opq_decode", header, re.S)
    assert "acc = fmaf(x[i, b], R[a, b], acc) for b = 0 .. d-1" in header        # the order of the arithmetic, where it is declared
    assert "blocks of 4096 rows" in header
    assert _lib.load().wise_abi_version() == 5
    # refusals that need no device: shapes are checked before anything is launched
    lib = _lib.load()
    assert lib.wise_opq_rotate(0, 0, 1, 1028, 0, 0) == -3 and b"d <= 1024" in lib.wise_last_error()
    assert lib.wise_opq_rotate(0, 0, 1, 510, 0, 0) == -3
    assert lib.wise_opq_corr_workspace_bytes(70000, 512) == 18 * 512 * 512 * 8 and lib.wise_opq_corr_workspace_bytes(0, 64) == 64 * 64 * 8
    assert lib.wise_opq_corr_workspace_bytes(10, 2048) == 0
    assert lib.wise_opq_corr(0, 0, 0, 1, 512, 7, 0, 0, 0, 0) == -3
    assert lib.wise_opq_decode(0, 0, 0, 0, 0, 1, 0, 0, 0, 2048, 64, 0, 0) == -3


def test_opq_operators_are_registered_and_infer_shapes():
    import torch

    import wise_amd.torch_ops  # noqa: F401

    y = torch.ops.wise_hip.opq_rotate(torch.empty(7, 64, device="meta"), torch.empty(64, 64, device="meta"))
    assert y.shape == (7, 64) and y.dtype == torch.float32
    M = torch.ops.wise_hip.opq_corr(torch.empty(9, 8, dtype=torch.uint8, device="meta"), torch.empty(8, 256, 8, device="meta"),
                                    torch.empty(9, 64, device="meta"))
    assert M.shape == (64, 64) and M.dtype == torch.float64
    with pytest.raises((NotImplementedError, RuntimeError)):      # no CPU kernel behind it
        torch.ops.wise_hip.opq_rotate(torch.zeros(2, 8), torch.eye(8))

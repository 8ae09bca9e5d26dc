"""IndexIVFSQ8 without a GPU: the float32 restatement (tests/ivfsq_ref.py) against float64, the quantizer's properties, the
'IwSq' file, the index-type names, the recorded recall study, and the entry points as the header declares them."""
import json
import re
import struct
from pathlib import Path

import numpy as np
import pytest

import ivfsq_ref as sq
from wise_amd import _lib
from wise_amd.index import faiss_io
from wise_amd.index.feature_search_index import parse_ivfpq_type

ROOT = Path(__file__).resolve().parent.parent


def unit_rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def small_index(N=700, d=48, nlist=9, seed=3):
    """(centroids, vmin, vdiff, codes, ids, list_off, resid) of N rows grouped into nlist lists (list 4 empty), with duplicated rows"""
    rng = np.random.default_rng(seed)
    c = unit_rows(nlist, d, seed + 1)
    X = unit_rows(N, d, seed + 2)
    X[N // 2:N // 2 + 40] = X[:40]                               # equal rows: equal scores wherever they share a list
    a = (X @ c.T).argmax(axis=1)
    a[a == 4] = 5
    order = np.argsort(a, kind="stable")
    X, a = X[order], a[order]
    list_off = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=nlist))]).astype(np.int64)
    resid = (X - c[a]).astype(np.float32)
    vmin, vdiff = sq.train(resid)
    ids = rng.permutation(N).astype(np.int64) * 3 + 11
    return c, vmin, vdiff, sq.encode(resid, vmin, vdiff), ids, list_off, resid


def test_fma32_is_the_correctly_rounded_fused_multiply_add():
    from fractions import Fraction

    rng = np.random.default_rng(0)
    n = 3000
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-12, 12, n)).astype(np.float32)
    b = rng.integers(0, 256, n).astype(np.float32)
    c = (rng.standard_normal(n) * 10.0 ** rng.integers(-12, 12, n)).astype(np.float32)
    got = sq.fma32(a, b, c)
    for i in range(n):
        v = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        f = np.float32(float(v))
        cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
        best = min(cands, key=lambda x: (abs(Fraction(float(x)) - v), int(np.float32(x).view(np.uint32)) & 1))
        assert best.view(np.uint32) == got[i].view(np.uint32), (a[i], b[i], c[i])
    one = np.ones(1, np.float32)
    assert sq.fma32(np.array([2.0 ** -24], np.float32), one, one)[0] == np.float32(1.0)                       # an exact tie: to even
    assert sq.fma32(np.array([2.0 ** -24 * (1 + 2.0 ** -20)], np.float32), one, one)[0] == np.float32(1 + 2.0 ** -23)   # just above it


@pytest.mark.parametrize("d", [16, 48, 128, 512])
def test_restatement_is_within_the_summation_bound_of_float64(d):
    """score (float32, the scan's order) against float64 q . x^ with x^ = c_l + vmin + vdiff (code + 0.5) / 255 evaluated in float64:
    |delta| <= gamma (|bias| + |q0| + sum |w_i| 255), gamma = (d + 2) 2^-24 / (1 - (d + 2) 2^-24) — the bound for a sum of
    d + 2 float32 terms.  Derived, not measured."""
    c, vmin, vdiff, codes, ids, list_off, _ = small_index(N=600, d=d, seed=d)
    nlist = len(c)
    Q = unit_rows(5, d, d + 7) * np.float32(1.7)
    coarse = Q.astype(np.float64) @ c.astype(np.float64).T
    bias = coarse.astype(np.float32)
    W, q0 = sq.query(Q, vmin, vdiff)
    xhat = sq.decode_rows(codes, list_off, c, vmin, vdiff, np.float64)
    lists = sq.list_of_rows(list_off)
    u = (d + 2) * 2.0 ** -24
    gamma = u / (1 - u)
    worst = 0.0
    for q in range(len(Q)):
        s = (bias[q, lists] + q0[q]).astype(np.float32) + sq.row_sums(codes, W[q])
        assert s.dtype == np.float32
        ref = xhat @ Q[q].astype(np.float64)
        bound = gamma * (np.abs(bias[q, lists]).astype(np.float64) + abs(float(q0[q])) + 255.0 * np.abs(W[q]).astype(np.float64).sum())
        delta = np.abs(s.astype(np.float64) - ref)
        worst = max(worst, float((delta / bound).max()))
        assert (delta <= bound).all(), (d, q, float((delta / bound).max()))
    print(f"d={d}: largest |delta| / bound = {worst:.4f}")
    assert nlist == 9


def _quantizer_case():
    d, n = 32, 4000
    rng = np.random.default_rng(5)
    resid = (rng.standard_normal((n, d)) * rng.uniform(0.01, 3.0, d)).astype(np.float32)
    resid[:, 7] = np.float32(0.25)                                # a dimension that never varies
    vmin, vdiff = sq.train(resid)
    return resid, vmin, vdiff, sq.encode(resid, vmin, vdiff)


def test_encode_decode_error_is_half_a_bin():
    """|x^ - r| <= vdiff[i] / 510 * (1 + 2^-20) per dimension for rows inside the trained range, x^ the decoder's formula
    vmin + vdiff (code + 0.5) / 255 evaluated in float64: the statement is about the bin the encoder picks.  It holds because the
    encoder evaluates its formula in float64 — the bin is then the one the real number falls into up to ~1e-13 of a bin, where
    half a bin times 2^-20 is 4.8e-7 of one.  (An encoder in float32 rounds r - vmin, 255 / vdiff and their product and misses
    the bound by up to 3.2e-5 on these rows.)  What the float32 DECODER adds is its own rounding, bounded in the test below."""
    resid, vmin, vdiff, codes = _quantizer_case()
    live = vdiff > 0
    err = np.abs(sq.decode(codes, vmin, vdiff, np.float64) - resid.astype(np.float64))[:, live]
    half = vdiff.astype(np.float64)[live][None, :] / 510.0
    print(f"largest error = vdiff / 510 * (1 + {float((err / half).max() - 1.0):.3e})")
    assert (err <= half * (1 + 2.0 ** -20)).all()
    # the rows that set the range sit in the first and the last bin
    assert (codes[resid.argmin(axis=0), np.arange(resid.shape[1])] == 0).all()
    assert (codes[resid.argmax(axis=0)[live], np.arange(resid.shape[1])[live]] >= 254).all()


def test_float32_decoder_is_within_its_rounding_of_the_formula():
    """The decoder's three float32 operations against the same formula in float64, u = 2^-24: xi = fl((code + 0.5) / 255) <= 1.002
    is off by u xi, s = fl(xi vdiff) by that times vdiff plus u s, y = fl(vmin + s) by u |y|: in all at most
    u (|vmin| + 4 vdiff).  Derived, not measured."""
    resid, vmin, vdiff, codes = _quantizer_case()
    delta = np.abs(sq.decode(codes, vmin, vdiff).astype(np.float64) - sq.decode(codes, vmin, vdiff, np.float64))
    bound = 2.0 ** -24 * (np.abs(vmin).astype(np.float64) + 4.0 * vdiff.astype(np.float64))
    assert (delta <= bound[None, :]).all()


def test_clamping_and_constant_dimensions():
    resid, vmin, vdiff, codes = _quantizer_case()
    assert vdiff[7] == 0 and vmin[7] == np.float32(0.25)
    assert np.array_equal(vmin, resid.min(axis=0)) and np.array_equal(vdiff, resid.max(axis=0) - resid.min(axis=0))
    assert codes.dtype == np.uint8 and codes.min() == 0 and codes.max() == 255
    dec = sq.decode(codes, vmin, vdiff)
    assert dec.dtype == np.float32
    assert (codes[:, 7] == 0).all() and (dec[:, 7] == vmin[7]).all()  # vdiff == 0: code 0, decoded to vmin
    # rows outside the trained range clamp
    out = np.stack([vmin - np.float32(1.0), vmin + vdiff + np.float32(1.0), vmin - np.float32(1e6), vmin + np.float32(1e6)])
    co = sq.encode(out, vmin, vdiff)
    live = vdiff > 0
    assert (co[0] == 0).all() and (co[2] == 0).all()
    assert (co[1][live] == 255).all() and (co[3][live] == 255).all() and (co[1][~live] == 0).all()


@pytest.mark.parametrize("d", [16, 48])
def test_scan_with_every_list_probed_is_brute_force_over_the_decoded_rows(d):
    c, vmin, vdiff, codes, ids, list_off, _ = small_index(N=700, d=d, seed=10 + d)
    nlist, N = len(c), len(codes)
    Q = unit_rows(4, d, 99)
    bias = (Q.astype(np.float64) @ c.astype(np.float64).T).astype(np.float32)
    W, q0 = sq.query(Q, vmin, vdiff)
    probes = np.tile(np.arange(nlist, dtype=np.int64), (len(Q), 1))
    lists = sq.list_of_rows(list_off)
    for k in (1, 10, N + 5):
        D, I = sq.scan(codes, list_off, None, W, q0, probes, bias, k)
        for q in range(len(Q)):
            s = (bias[q, lists] + q0[q]).astype(np.float32) + sq.row_sums(codes, W[q])      # every row's score, brute force
            order = np.lexsort((np.arange(N), -sq.f32_order(s)))[:k]
            assert np.array_equal(I[q, :len(order)], order) and np.array_equal(D[q, :len(order)].view(np.uint32), s[order].view(np.uint32))
            assert (I[q, len(order):] == -1).all() and (D[q, len(order):] == sq.NEG).all()
    # equal rows in one list: equal scores, the first in list order comes first
    D, I = sq.scan(codes, list_off, None, W, q0, probes, bias, N)
    for q in range(len(Q)):
        same = np.flatnonzero(D[q, 1:].view(np.uint32) == D[q, :-1].view(np.uint32))
        assert len(same) > 0 and (I[q, same] < I[q, same + 1]).all()
    # ids are looked up at the end; a skipped probe and a probe past nlist contribute nothing
    probes2 = probes.copy()
    probes2[:, 0] = -1
    D2, I2 = sq.scan(codes, list_off, ids, W, q0, probes2, bias, 10)
    keep = np.ones(N, bool)
    keep[list_off[0]:list_off[1]] = False
    D3, I3 = sq.scan(codes, list_off, ids, W, q0, probes, bias, 10, keep=keep)
    assert np.array_equal(I2, I3) and np.array_equal(D2.view(np.uint32), D3.view(np.uint32))


def test_ivf_sq_file_round_trip(tmp_path):
    c, vmin, vdiff, codes, ids, list_off, _ = small_index(N=500, d=16, nlist=9)
    trained = np.concatenate([vmin, vdiff])
    fn = tmp_path / "video-IndexIVFSQ8.faiss"
    faiss_io.write_ivf_sq_ip(fn, c, trained, codes, ids, list_off, nprobe=17)
    assert faiss_io.index_fourcc(fn) == "IwSq"
    assert b"full" in fn.read_bytes()
    f = faiss_io.read_ivf_sq_ip(fn)
    assert np.array_equal(f["centroids"], c) and np.array_equal(f["trained"].view(np.uint32), trained.view(np.uint32))
    assert f["codes"].dtype == np.uint8 and f["codes"].tobytes() == codes.tobytes()
    assert np.array_equal(f["ids"], ids) and np.array_equal(f["list_off"], list_off) and f["nprobe"] == 17
    assert np.array_equal(np.diff(f["list_off"]), np.diff(list_off))
    # the record after the direct map: qtype QT_8bit, RS_minmax, argument 0, d, code_size, 2 d trained values
    raw = fn.read_bytes()
    at = 4 + 33 + 16 + 4 + 33 + 8 + 4 * c.size + 9
    assert struct.unpack_from("<iifQQQ", raw, at) == (0, 0, 0.0, 16, 16, 32)
    assert struct.unpack_from("<QB", raw, at + 36 + 4 * 32) == (16, 1)
    # every other reader refuses it, and it refuses the other files
    for reader in (faiss_io.read_ivf_flat_ip, faiss_io.read_ivf_pq_ip, faiss_io.read_idmap_flat_ip):
        with pytest.raises(RuntimeError):
            reader(fn)
    flat = tmp_path / "video-IndexIVFFlat.faiss"
    faiss_io.write_ivf_flat_ip(flat, c, np.zeros((500, 16), np.float32), ids, list_off)
    with pytest.raises(RuntimeError, match="IndexIVFScalarQuantizer"):
        faiss_io.read_ivf_sq_ip(flat)
    # a file cut short is refused wherever the cut falls: in the lists, in the trained values, in the header
    for cut in (len(raw) - 1, len(raw) - 8 * 500 - 3, at + 40, 20):
        short = tmp_path / f"cut-{cut}.faiss"
        short.write_bytes(raw[:cut])
        with pytest.raises(RuntimeError):
            faiss_io.read_ivf_sq_ip(short)
    # most lists empty: the sparse size table
    off2 = np.array([0] * 9 + [500], dtype=np.int64)
    faiss_io.write_ivf_sq_ip(fn, c, trained, codes, ids, off2)
    assert struct.unpack_from("<I", fn.read_bytes(), at + 36 + 4 * 32 + 9 + 20)[0] == faiss_io._fourcc("sprs")
    f = faiss_io.read_ivf_sq_ip(fn)
    assert np.array_equal(f["list_off"], off2) and f["codes"].tobytes() == codes.tobytes() and np.array_equal(f["ids"], ids) and f["nprobe"] == 1
    with pytest.raises(RuntimeError):
        faiss_io.read_ivf_sq_ip(tmp_path / "missing.faiss")


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

    assert parse_ivfpq_type("IndexIVFSQ8", 512) is None and parse_ivfpq_type("IndexIVFSQ8") is None
    si = _store(tmp_path, 64)
    for bad in ("IndexIVFSQ4", "IndexIVFSQ"):
        with pytest.raises(NotImplementedError, match="IndexFlatIP, IndexIVFFlat and IndexIVFPQ<m>"):
            si.create_index(bad)                                  # refused before the store is opened or a GPU is touched
        assert not si.get_index_filename(bad).exists()
    assert si.get_index_filename("IndexIVFSQ8").name == "video-IndexIVFSQ8.faiss"

    class Accepted(Exception):
        pass

    class StandIn:                                                # the name reaches the index class: no GPU here
        def __init__(self, d, nlist):
            raise Accepted(f"{d} {nlist}")

    monkeypatch.setattr(fsi, "IVFSQIPIndex", StandIn)
    with pytest.raises(Accepted, match="64 "):
        si.create_index("IndexIVFSQ8")
    # a dimension the kernels do not serve is refused before a row is read
    si40 = _store(tmp_path / "b", 40)
    with pytest.raises(ValueError, match="multiple of 16"):
        si40.create_index("IndexIVFSQ8")


def test_recorded_recall_study_first_seed():
    gold = json.loads((ROOT / "tests" / "golden" / "ivfsq_quality.json").read_text())
    assert gold["seeds"][0] == 0 and json.dumps(sq.STUDY) in gold["what"]
    run = sq.recall_study(gold["seeds"][0])
    assert run == gold["runs"][0], (run, gold["runs"][0])
    assert gold["sq8_min"] == min(r["sq8"] for r in gold["runs"]) and gold["gap_max"] == max(r["ivfflat"] - r["sq8"] for r in gold["runs"])


def test_header_declares_and_library_exports_the_sq_entry_points():
    from wise_amd.build import HIP_SOURCES, declared_symbols

    assert "ivf_sq.hip" in HIP_SOURCES
    names = ["wise_sq_train", "wise_sq_encode", "wise_sq_query", "wise_sq_decode", "wise_ivfsq_scan_workspace_bytes",
             "wise_ivfsq_scan", "wise_ivfsq_scan_sel"]
    lib = _lib.load()
    for name in names:
        assert name in declared_symbols() and name in _lib.SIGNATURES
        assert getattr(lib, name) is not None                    # exported by the built library: the version script follows the header
    assert [len(_lib.SIGNATURES[n][1]) for n in names] == [5, 6, 7, 11, 3, 18, 19]
    header = (ROOT / "include" / "wise_hip.h").read_text()
    for name, (_, args) in ((n, _lib.SIGNATURES[n]) for n in names):
        decl = re.search(r"\b(?:int|size_t)\s+" + name + r"\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == len(args), name
    assert lib.wise_abi_version() == 5
    assert lib.wise_ivfsq_scan_workspace_bytes(3, 5, 10) == 1280 and lib.wise_ivfsq_scan_workspace_bytes(1, 1, 4096) == 0
    from wise_amd.index import IVFSQIPIndex
    from wise_amd.index.ivf_sq import IVFSQIPIndex as direct
    assert IVFSQIPIndex is direct

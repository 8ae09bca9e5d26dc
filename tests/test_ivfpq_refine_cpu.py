"""IndexIVFPQ<m>R8 / R16 without a GPU: the numpy restatement of the re-ranking stage (tests/ivfpq_refine_ref.py) against float64
brute force and the flat oracle, the seeded recall study, the 'WiPR' file round trip, the type names and the header's symbols."""
import json
import re
from pathlib import Path

import numpy as np
import pytest

import ivfpq_refine_ref as rr
from oracle import ip_topk_ref
from wise_amd.index import faiss_io
from wise_amd.index.feature_search_index import parse_ivfpq_refine_type, parse_ivfpq_type

ROOT = Path(__file__).resolve().parent.parent
TOL = 2e-5      # the project's search tolerance


def unit_rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def check_against(D, I, Do, Io, tol=TOL):
    assert D.shape == Do.shape and I.dtype == np.int64
    assert np.allclose(D, Do, atol=tol)
    gap_ok = np.ones_like(Io, dtype=bool)
    gap_ok[:, 1:] &= (Do[:, :-1] - Do[:, 1:]) > tol
    gap_ok[:, :-1] &= (Do[:, :-1] - Do[:, 1:]) > tol
    assert np.array_equal(I[gap_ok], Io[gap_ok])


def test_quantisers_are_what_the_builders_document():
    X = unit_rows(50, 32, 0) * np.linspace(0.1, 30, 50, dtype=np.float32)[:, None]
    X[7] = 0
    q, s = rr.quantise_i8(X)
    assert q.dtype == np.int8 and s.dtype == np.float32
    assert np.array_equal(s, np.abs(X).max(axis=1) / np.float32(127))
    assert (np.abs(q).max(axis=1)[np.arange(50) != 7] == 127).all() and not q[7].any() and s[7] == 0
    # half a step per component, plus the float32 rounding of x * (127 / max) and of scale * code
    err = np.abs(rr.dequantise(q, 8, s).astype(np.float64) - X)
    assert (err <= (0.5 + 127 * 2.0 ** -22) * s[:, None].astype(np.float64)).all()
    b = rr.quantise_bf16(X)
    back = rr.dequantise(b, 16)
    assert b.dtype == np.uint16 and (np.abs(back - X) <= np.abs(X) * 2.0 ** -8).all()      # round to nearest: half of 2^-7 |x|
    assert np.array_equal(rr.quantise_bf16(back), b)                                       # a bf16 value is kept as it is
    # ties go to even: 1 + 2^-8 lies halfway between 1 and 1 + 2^-7
    assert rr.quantise_bf16(np.array([[1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8]], dtype=np.float32)).tolist() == [[0x3F80, 0x3F82]]


@pytest.mark.parametrize("kind", [8, 16])
@pytest.mark.parametrize("d", [16, 128, 768])
def test_scores_within_the_chain_bound_of_float64(kind, d):
    """The float32 chain against float64 dot products over the SAME dequantised rows.  A chain of d products and d - 1 sums
    (+ the product by the scale, kind 8) carries at most gamma_n = n u / (1 - n u) of sum |q_i x_i|, u = 2^-24, n = d (+ 1)
    (Higham, Accuracy and Stability, section 3.1), and sum |q_i x_i| <= |q| |x| (Cauchy-Schwarz); float64's own error and the
    rounding of scale * code in `dequantise` (u |x|, kind 8) are added."""
    N, nq = 400, 5
    X = unit_rows(N, d, d + kind) * np.random.default_rng(1).uniform(0.5, 2.0, (N, 1)).astype(np.float32)
    Q = unit_rows(nq, d, 3) * np.float32(1.7)
    rows, scales = rr.quantise(X, kind)
    Xd = rr.dequantise(rows, kind, scales).astype(np.float64)
    u, n = 2.0 ** -24, d + (1 if kind == 8 else 0)
    gamma = n * u / (1 - n * u)
    for q in range(nq):
        got = rr.scores(rows, kind, scales, Q[q]).astype(np.float64)
        want = Xd @ Q[q].astype(np.float64)
        bound = (gamma + (u if kind == 8 else 0) + d * 2.0 ** -52) * np.linalg.norm(Q[q].astype(np.float64)) * np.linalg.norm(Xd, axis=1) \
            * (1 + u)
        err = np.abs(got - want)
        print(f"kind {kind} d {d} q {q}: max err {err.max():.3e}, max err / bound {np.max(err / bound):.3f}")
        assert (err <= bound).all()


@pytest.mark.parametrize("kind", [8, 16])
def test_lossless_store_with_every_row_a_candidate_equals_the_flat_oracle(kind):
    N, d, k = 1500, 64, 10
    rng = np.random.default_rng(kind)
    if kind == 8:      # rows that ARE scale * integers: codes in [-127, 127] with a 127 in every row, scales powers of two
        codes = rng.integers(-127, 128, (N, d))
        codes[np.arange(N), rng.integers(0, d, N)] = 127
        X = (codes * 2.0 ** rng.integers(-12, -8, (N, 1))).astype(np.float32)
    else:              # rows that are bf16 values
        X = rr.dequantise(rr.quantise_bf16(unit_rows(N, d, 5)), 16)
    rows, scales = rr.quantise(X, kind)
    assert np.array_equal(rr.dequantise(rows, kind, scales), X)
    ids = rng.permutation(N).astype(np.int64) * 3 + 1
    Q = unit_rows(6, d, 9)
    cand = np.tile(np.arange(N, dtype=np.int64), (Q.shape[0], 1))
    D, I = rr.refine(rows, kind, scales, ids, Q, cand, k)
    Df, If = ip_topk_ref.ip_topk(X, Q, k, ids=ids)
    check_against(D, I, Df, If)


def test_refine_restatement_holes_ties_and_padding():
    d, k = 16, 6
    X = unit_rows(8, d, 1)
    X[5] = X[2]
    X[6] = X[2]                                                        # three equal rows: equal scores
    Q = X[2:3].copy()
    for kind in (8, 16):
        rows, scales = rr.quantise(X, kind)
        cand = np.array([[6, -1, 2, 7, 99, 5, -1, 0]], dtype=np.int64)  # holes and a position past the end are skipped
        D, I = rr.refine(rows, kind, scales, None, Q, cand, k)
        assert I[0, :3].tolist() == [2, 5, 6] and D[0, 0] == D[0, 1] == D[0, 2]          # ties: the lower position first
        assert sorted(I[0, 3:5].tolist()) == [0, 7] and I[0, 5] == -1 and D[0, 5] == rr.NEG
        ids = np.arange(8, dtype=np.int64) * 10 + 3
        assert np.array_equal(rr.refine(rows, kind, scales, ids, Q, cand, k)[1][0, :5], ids[I[0, :5]])
        Dn, In = rr.refine(rows, kind, scales, None, Q, np.full((1, 4), -1, dtype=np.int64), k)
        assert (In == -1).all() and (Dn == rr.NEG).all()


def test_the_k_best_are_the_first_k_of_the_kc_best():
    """What tests/test_gpu_ivfpq_refine.py uses to take the answers for several k from one run of the restatement."""
    N, d, kc = 600, 32, 100
    X = unit_rows(N, d, 4)
    X[300:330] = X[7]
    Q = unit_rows(3, d, 5)
    rng = np.random.default_rng(6)
    cand = np.stack([rng.permutation(N)[:kc] for _ in range(3)]).astype(np.int64)
    cand[rng.random(cand.shape) < 0.2] = -1
    for kind in (8, 16):
        rows, scales = rr.quantise(X, kind)
        Dfull, Ifull = rr.refine(rows, kind, scales, None, Q, cand, kc)
        for k in (1, 10, 150):
            D, I = rr.refine(rows, kind, scales, None, Q, cand, k)
            assert np.array_equal(D[:, :kc], Dfull[:, :k]) and np.array_equal(I[:, :kc], Ifull[:, :k])
            assert (I[:, kc:] == -1).all() and (D[:, kc:] == rr.NEG).all()


def test_recall_study_on_one_more_seed(golden_dir):
    """The study of the issue as a seeded test: on clustered rows (the bench tool's recipe, 60,000 x 128, 244 lists, m = 16,
    nprobe 32, k = 10, 64 queries) re-ranking the 10 * 50 best PQ positions must lift recall@10 over the PQ scan alone by at
    least the smallest gain the restatement showed on five other seeds, less the spread of that gain
    (tests/golden/ivfpq_refine_quality.json, written by `python tests/ivfpq_refine_ref.py`).  The golden file also records the
    ceilings: every probed row re-ranked by the int8 rows, the bf16 rows and the fp32 rows.
    Recorded (five seeds): PQ alone 0.20 - 0.24; k_factor 50: R8 0.927 - 0.947, R16 0.967 - 0.977; k_factor 100 adds at most 0.002."""
    gold = json.loads((golden_dir / "ivfpq_refine_quality.json").read_text())
    assert 5 not in gold["seeds"] and len(gold["runs"]) == 5
    assert {k: v for k, v in gold.items() if k.startswith("gain_")} == rr.study_summary(gold["runs"])
    cfg = dict(rr.STUDY, k_factors=(50,))
    r = rr.recall_study(5, cfg)
    print(json.dumps(r))
    for kind in (8, 16):
        gain = r[f"r{kind}"]["50"] - r["pq_alone"]
        floor = gold[f"gain_min_r{kind}"] - gold[f"gain_spread_r{kind}"]
        print(f"R{kind}: gain {gain:.4f}, floor {floor:.4f}")
        assert floor > 0.3 and gain >= floor
    # The issue expected the 16-bit store to close the gap the int8 store leaves to the fp32 rows.  It does not: on the five
    # recorded seeds the ceilings are 0.927 - 0.947 (int8), 0.967 - 0.978 (bf16) and 1.0 (fp32) — bf16 halves the gap.  What
    # is held here is the order only: a finer store never ranks worse.
    for run in gold["runs"] + [r]:
        assert run["ceiling_r8"] <= run["ceiling_r16"] <= run["ceiling_fp32"]


def test_refine_type_names():
    assert parse_ivfpq_refine_type("IndexIVFPQ64R8", 512) == (64, 8)
    assert parse_ivfpq_refine_type("IndexIVFPQ16R16", 512) == (16, 16)
    assert parse_ivfpq_refine_type("IndexIVFPQ96R16", 768) == (96, 16)
    assert parse_ivfpq_refine_type("IndexIVFPQR8", 512) == (128, 8)            # bare: m = d / 4, as IndexIVFPQ
    assert parse_ivfpq_refine_type("IndexIVFPQ64R8") == (64, 8)
    with pytest.raises(ValueError):
        parse_ivfpq_refine_type("IndexIVFPQ7R8", 512)                          # bad m: d % m
    with pytest.raises(ValueError):
        parse_ivfpq_refine_type("IndexIVFPQ192R8", 768)                        # bad m: > 128
    with pytest.raises(ValueError, match="R8 .* R16"):
        parse_ivfpq_refine_type("IndexIVFPQ64R4", 512)                         # bad kind
    with pytest.raises(ValueError, match="R8 .* R16"):
        parse_ivfpq_refine_type("IndexIVFPQ64R32")
    with pytest.raises(ValueError, match="multiple of 16"):
        parse_ivfpq_refine_type("IndexIVFPQ6R8", 24)                           # the int8 builder takes d % 16 == 0
    assert parse_ivfpq_refine_type("IndexIVFPQ6R16", 24) == (6, 16)
    for other in ("IndexFlatIP", "IndexIVFFlat", "IndexIVFPQ64", "IndexIVFPQ", "IndexIVFPQ64R", "IndexIVFPQ64Rx", "IndexIVFPQxR8",
                  "IndexHNSWFlat", "IndexIVFPQ64R-8"):
        assert parse_ivfpq_refine_type(other, 512) is None
    # the old parser does not know the new names, and keeps its answers for its own
    for new in ("IndexIVFPQ64R8", "IndexIVFPQ64R16", "IndexIVFPQR8"):
        assert parse_ivfpq_type(new, 512) is None
    assert parse_ivfpq_type("IndexIVFPQ64", 512) == 64 and parse_ivfpq_type("IndexIVFPQ", 512) == 128


def small_refine_index(kind, N=500, d=16, m=4, nlist=9, seed=0):
    rng = np.random.default_rng(seed)
    c = unit_rows(nlist, d, seed + 1)
    X = unit_rows(N, d, seed + 2)
    a = np.sort(rng.integers(0, nlist, N))
    list_off = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=nlist))]).astype(np.int64)
    cb = (0.1 * rng.standard_normal((m, 256, d // m))).astype(np.float32)
    codes = rng.integers(0, 256, (N, m)).astype(np.uint8)
    rows, scales = rr.quantise(X, kind)
    return c, cb, codes, np.arange(N, dtype=np.int64) * 3 + 7, list_off, rows, scales


@pytest.mark.parametrize("kind", [8, 16])
def test_refine_file_round_trip(tmp_path, kind):
    c, cb, codes, ids, list_off, rows, scales = small_refine_index(kind)
    fn = tmp_path / f"video-IndexIVFPQ4R{kind}.faiss"
    faiss_io.write_ivf_pq_refine_ip(fn, c, cb, codes, ids, list_off, kind, 37, rows, scales, nprobe=17)
    assert faiss_io.index_fourcc(fn) == "WiPR"
    f = faiss_io.read_ivf_pq_refine_ip(fn)
    assert f["kind"] == kind and f["k_factor"] == 37 and f["nprobe"] == 17
    assert np.array_equal(f["centroids"], c) and np.array_equal(f["codebooks"], cb) and np.array_equal(f["codes"], codes)
    assert np.array_equal(f["ids"], ids) and np.array_equal(f["list_off"], list_off)
    assert f["rows"].dtype == rows.dtype and np.array_equal(f["rows"], rows)
    assert (f["scales"] is None) if kind == 16 else (f["scales"].dtype == np.float32 and np.array_equal(f["scales"], scales))
    assert fn.stat().st_size == 16 + _pq_file_size(tmp_path, c, cb, codes, ids, list_off) + 8 + rows.nbytes + (8 + 4 * len(ids) if kind == 8 else 0)
    for reader in (faiss_io.read_ivf_pq_ip, faiss_io.read_ivf_flat_ip, faiss_io.read_idmap_flat_ip):      # nobody else takes it
        with pytest.raises(RuntimeError):
            reader(fn)
    pq = tmp_path / "video-IndexIVFPQ4.faiss"
    faiss_io.write_ivf_pq_ip(pq, c, cb, codes, ids, list_off)
    with pytest.raises(RuntimeError):
        faiss_io.read_ivf_pq_refine_ip(pq)
    # most lists empty: the sparse size table inside the record
    off2 = np.array([0] * 9 + [500], dtype=np.int64)
    faiss_io.write_ivf_pq_refine_ip(fn, c, cb, codes, ids, off2, kind, 1, rows, scales)
    f = faiss_io.read_ivf_pq_refine_ip(fn)
    assert np.array_equal(f["list_off"], off2) and np.array_equal(f["rows"], rows) and f["k_factor"] == 1 and f["nprobe"] == 1


def _pq_file_size(tmp_path, c, cb, codes, ids, list_off):
    fn = tmp_path / "plain.faiss"
    faiss_io.write_ivf_pq_ip(fn, c, cb, codes, ids, list_off, nprobe=17)
    return fn.stat().st_size


def test_header_declares_the_refine_entry_points():
    from wise_amd import _lib
    from wise_amd.build import declared_symbols

    header = (ROOT / "include" / "wise_hip.h").read_text()
    for name in ("wise_ivf_refine", "wise_ivf_refine_rows"):
        assert name in declared_symbols() and name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert len(_lib.SIGNATURES["wise_ivf_refine"][1]) == 14
    # ABI 5, listed as added within it; the order of the arithmetic is spelled out where the entry is declared
    assert re.search(r"added within 5:.*wise_ivf_refine and wise_ivf_refine_rows\)", header, re.S)
    assert "acc = acc + (Q[q,i] * x_i) for i = 0 .. d-1" in header
    assert _lib.load().wise_abi_version() == 5


def test_refine_operator_is_registered_and_infers_shapes():
    import torch

    import wise_amd.torch_ops  # noqa: F401

    assert "Tensor? scales" in str(torch.ops.wise_hip.ivf_refine.default._schema)
    D, I = torch.ops.wise_hip.ivf_refine(torch.empty(100, 64, dtype=torch.int8, device="meta"), torch.empty(100, device="meta"), None,
                                         torch.empty(3, 64, device="meta"), torch.empty(3, 50, dtype=torch.int64, device="meta"), 10)
    assert D.shape == (3, 10) and D.dtype == torch.float32 and I.shape == (3, 10) and I.dtype == torch.int64
    with pytest.raises((NotImplementedError, RuntimeError)):      # no CPU kernel behind it
        torch.ops.wise_hip.ivf_refine(torch.zeros(4, 16, dtype=torch.int8), torch.ones(4), None, torch.zeros(1, 16),
                                      torch.zeros(1, 2, dtype=torch.int64), 1)

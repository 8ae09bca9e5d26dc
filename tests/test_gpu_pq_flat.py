"""-m gpu: IndexPQ<m> and its R8 / R16 forms — wise_pqflat_topk / _topk_pos / _decode through the C ABI, then the classes of
wise_amd/index/flat_pq.py and the plugin, every result bit for bit against the numpy restatement (tests/pq_flat_ref.py):
(1) the scan over every load width, pass size and block geometry, ties and tables that round together, and the same bits from
wise_ivfpq_scan over one list; (2) the scan over positions; (3) decode; (4) refusals; (5) graph capture; (6) the classes; (7) the
plugin's files."""
import hashlib

import numpy as np
import pytest
import torch

import ivfpq_ref
import ivfpq_refine_ref
import pq_flat_ref as ref
from wise_amd import _lib

pytestmark = pytest.mark.gpu

NEG = np.float32(-3.4028234663852886e38)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def block_rows(m, nq, k):
    """B, the rows one block of the first pass takes before the next block's rows begin: 64 x the waves plan_pass
    (csrc/pq_flat.hip) gives a block — restated here so that the sizes around a block boundary are tested for every geometry."""
    cap = 1
    while cap < k + 64:
        cap <<= 1
    fits = lambda q, w: q * m * 1024 + w * q * cap * 8 <= 160 * 1024
    q = 4
    while q > nq:
        q >>= 1
    while q > 1 and not fits(q, 4):
        q >>= 1
    w = 16
    while w > 1 and not fits(q, w):
        w >>= 1
    assert fits(q, w)
    return 64 * w


def gpu_topk(Cd, N, m, Ld, k, ids=None, id_base=0, pos=None, ws_bytes=None):
    lib = _lib.lib()
    nq = Ld.shape[0]
    n = N if pos is None else pos.numel()
    need = lib.wise_pqflat_topk_workspace_bytes(n, m, nq, k)
    assert need > 0
    ws = torch.empty(need if ws_bytes is None else ws_bytes, dtype=torch.uint8, device="cuda")
    D = torch.full((nq, k), float("nan"), dtype=torch.float32, device="cuda")
    I = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    if pos is None:
        rc = lib.wise_pqflat_topk(_lib.ptr(Cd), N, m, Ld.data_ptr(), nq, k, _lib.ptr(ids), id_base, D.data_ptr(), I.data_ptr(), ws.data_ptr(),
                                  ws.numel(), _lib.stream_ptr())
    else:
        rc = lib.wise_pqflat_topk_pos(_lib.ptr(Cd), N, m, pos.data_ptr(), n, Ld.data_ptr(), nq, k, _lib.ptr(ids), id_base, D.data_ptr(),
                                      I.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, D.cpu().numpy(), I.cpu().numpy()


def make_case(N, m, nq, seed):
    """codes with a tenth of the rows exact copies of row 0 (exact ties), a table of N(0, 1/m) entries, ids that are not positions"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, (N, m)).astype(np.uint8)
    if N:
        codes[rng.random(N) < 0.1] = codes[0]
    lut = (rng.standard_normal((nq, m, 256)) / np.sqrt(m)).astype(np.float32)
    ids = rng.permutation(N).astype(np.int64) * 5 + 3
    return codes, lut, ids


# ------------------------------------------------------------------------------------------------------------------ (1) the scan
COMBOS = [(1, 10), (2, 10), (3, 10), (4, 10), (5, 10), (9, 10), (5, 1), (5, 100), (5, 2048)]      # (nq, k)


@pytest.mark.parametrize("m", [1, 4, 8, 12, 16, 20, 48, 64, 128])
def test_scan_bit_for_bit(m):
    for c, (nq, k) in enumerate(COMBOS):
        B = block_rows(m, nq, k)
        for N in (0, 1, 63, 64, 65, 2 * B - 1, 2 * B + 1, 20011):
            codes, lut, ids = make_case(N, m, nq, 1000 * m + 10 * c + N % 7)
            explicit = (c + N) % 2 == 0
            Cd, Ld = (_dev(codes) if N else None), _dev(lut)
            rc, D, I = gpu_topk(Cd, N, m, Ld, k, ids=_dev(ids) if explicit and N else None, id_base=0 if explicit else 1000)
            assert rc == 0, _lib.load().wise_last_error()
            Dr, Ir = ref.scan(codes, ids if explicit else None, lut, k, id_base=1000)
            what = f"m={m} nq={nq} k={k} N={N} B={B} explicit={explicit}"
            assert _same(D, Dr), what
            assert np.array_equal(I, Ir), what
            if N < k:
                assert (I[:, N:] == -1).all() and (D[:, N:] == NEG).all(), what


@pytest.mark.parametrize("m", [4, 16, 64, 128])
def test_equal_rows_across_block_boundaries_go_to_the_lower_position(m):
    nq, k = 2, 10
    B = block_rows(m, nq, k)
    N = 3 * B + 5
    codes, lut, _ = make_case(N, m, nq, 77 + m)
    codes[codes.sum(axis=1) == 0] = 1                       # no accidental copy of the winning row
    lut[:, :, 0] = np.float32(3.0)                          # the row of zeros scores 3 m: more than any other
    twins = [0, B - 1, B, 2 * B - 1, 2 * B, N - 1]          # both sides of two block boundaries, both ends
    codes[twins] = 0
    rc, D, I = gpu_topk(_dev(codes), N, m, _dev(lut), k)
    assert rc == 0
    assert np.array_equal(I[:, :6], np.tile(twins, (nq, 1))) and (D[:, :6] == D[:, :1]).all()
    Dr, Ir = ref.scan(codes, None, lut, k)
    assert _same(D, Dr) and np.array_equal(I, Ir)


def test_tables_with_negative_zero_and_sums_that_round_together():
    m, N, nq, k = 16, 5000, 3, 100
    rng = np.random.default_rng(5)
    values = np.array([-0.0, 0.0, 1.0, 1.0 + 2.0 ** -23, 2.0 ** 24, -2.0 ** 24, 0.5, 2.0 ** -30], dtype=np.float32)
    lut = values[rng.integers(0, len(values), (nq, m, 256))]
    lut[0] = np.float32(-0.0)                               # +0 + -0 + ... = +0: every row of query 0 ties at +0
    codes = rng.integers(0, 256, (N, m)).astype(np.uint8)
    rc, D, I = gpu_topk(_dev(codes), N, m, _dev(lut), k)
    assert rc == 0
    Dr, Ir = ref.scan(codes, None, lut, k)
    assert _same(D, Dr) and np.array_equal(I, Ir)
    assert _same(D[0], np.zeros(k, dtype=np.float32)) and np.array_equal(I[0], np.arange(k))      # +0, and the lowest positions
    assert (np.diff(D, axis=1) == 0).mean() > 0.2           # many exact ties among the sums


@pytest.mark.parametrize("m", [1, 4, 8, 12, 16, 20, 48, 64, 128])
def test_same_bits_as_the_list_scan_over_one_list(m):
    lib = _lib.lib()
    N, nq, k = 20011, 3, 10
    codes, lut, ids = make_case(N, m, nq, 31 + m)
    Cd, Ld, Id = _dev(codes), _dev(lut), _dev(ids)
    rc, D, I = gpu_topk(Cd, N, m, Ld, k, ids=Id)
    assert rc == 0
    off, probes, bias = _dev(np.array([0, N], dtype=np.int64)), _dev(np.zeros((nq, 1), dtype=np.int64)), _dev(np.zeros((nq, 1), dtype=np.float32))
    ws = torch.empty(lib.wise_ivfpq_scan_workspace_bytes(nq, 1, k, m), dtype=torch.uint8, device="cuda")
    D2 = torch.empty(nq, k, dtype=torch.float32, device="cuda")
    I2 = torch.empty(nq, k, dtype=torch.int64, device="cuda")
    _lib.check(lib.wise_ivfpq_scan(Cd.data_ptr(), N, m, off.data_ptr(), 1, Id.data_ptr(), Ld.data_ptr(), nq, probes.data_ptr(), bias.data_ptr(), 1,
                                   k, D2.data_ptr(), I2.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "wise_ivfpq_scan")
    torch.cuda.synchronize()
    assert _same(D, D2) and np.array_equal(I, I2.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------ (2) positions
@pytest.mark.parametrize("m", [12, 64])
def test_position_scan_equals_the_restatement_restricted(m):
    N, nq = 20011, 5
    codes, lut, ids = make_case(N, m, nq, 400 + m)
    rng = np.random.default_rng(m)
    Cd, Ld, Id = _dev(codes), _dev(lut), _dev(ids)
    chosen = {"all": np.arange(N), "tenth": np.sort(rng.permutation(N)[:N // 10]), "thousandth": np.sort(rng.permutation(N)[:N // 1000]),
              "one": np.array([N // 2]), "none": np.array([], dtype=np.int64)}
    for which, pos in chosen.items():
        pos = pos.astype(np.int64)
        for k, explicit in ((10, True), (100, False)):
            rc, D, I = gpu_topk(Cd, N, m, Ld, k, ids=Id if explicit else None, id_base=0 if explicit else 500, pos=_dev(pos))
            assert rc == 0, which
            Dr, Ir = ref.scan_pos(codes, ids if explicit else None, lut, pos, k, id_base=500)
            assert _same(D, Dr) and np.array_equal(I, Ir), f"{which} k={k}"
            if which == "all":                              # every position: the whole scan's answer
                De, Ie = ref.scan(codes, ids if explicit else None, lut, k, id_base=500)
                assert _same(D, De) and np.array_equal(I, Ie)
            if len(pos) < k:
                assert (I[:, len(pos):] == -1).all() and (D[:, len(pos):] == NEG).all()


# ------------------------------------------------------------------------------------------------------------------ (3) decode
@pytest.mark.parametrize("d,m", [(64, 16), (96, 1), (512, 64)])
def test_decode_is_exact_copies_and_nan_outside(d, m):
    lib = _lib.lib()
    N = 3000
    rng = np.random.default_rng(d + m)
    codes = rng.integers(0, 256, (N, m)).astype(np.uint8)
    cb = rng.standard_normal((m, 256, d // m)).astype(np.float32)
    pos = np.concatenate([rng.permutation(N)[:200], [0, N - 1, -1, N]]).astype(np.int64)
    out = torch.empty(len(pos), d, dtype=torch.float32, device="cuda")
    Cd, Pd, Bd = _dev(codes), _dev(pos), _dev(cb)
    _lib.check(lib.wise_pqflat_decode(Cd.data_ptr(), N, Pd.data_ptr(), len(pos), Bd.data_ptr(), d, m, out.data_ptr(), _lib.stream_ptr()),
               "wise_pqflat_decode")
    got = out.cpu().numpy()
    want = ref.decode(codes, pos, cb)
    assert _same(got[:-2], want[:-2]) and np.isnan(got[-2:]).all() and np.isnan(want[-2:]).all()


# ------------------------------------------------------------------------------------------------------------------ (4) refusals
def test_refusals_are_argument_checks_that_leave_the_outputs_untouched():
    lib = _lib.lib()
    N, m, nq, k = 1000, 16, 2, 10
    codes, lut, _ = make_case(N, m, nq, 9)
    Cd, Ld = _dev(codes), _dev(lut)
    ws = torch.empty(lib.wise_pqflat_topk_workspace_bytes(N, m, nq, 2048), dtype=torch.uint8, device="cuda")
    D = torch.full((nq, 2048), float("nan"), dtype=torch.float32, device="cuda")
    I = torch.full((nq, 2048), -7, dtype=torch.int64, device="cuda")
    pos = _dev(np.arange(10, dtype=np.int64))

    def call(m_, k_, ws_bytes):
        a = lib.wise_pqflat_topk(Cd.data_ptr(), N, m_, Ld.data_ptr(), nq, k_, 0, 0, D.data_ptr(), I.data_ptr(), ws.data_ptr(), ws_bytes, 0)
        b = lib.wise_pqflat_topk_pos(Cd.data_ptr(), N, m_, pos.data_ptr(), 10, Ld.data_ptr(), nq, k_, 0, 0, D.data_ptr(), I.data_ptr(),
                                     ws.data_ptr(), ws_bytes, 0)
        return a, b

    for m_, k_ in ((0, 10), (129, 10), (16, 0), (16, 2049)):
        assert lib.wise_pqflat_topk_workspace_bytes(N, m_, nq, k_) == 0
        assert call(m_, k_, ws.numel()) == (-3, -3)                       # WISE_E_UNSUPPORTED
    assert lib.wise_pqflat_topk_workspace_bytes(2 ** 32 - 1, m, nq, k) == 0 and lib.wise_pqflat_topk_workspace_bytes(-1, m, nq, k) == 0
    assert lib.wise_pqflat_topk_workspace_bytes(2 ** 32 - 2, 128, 1000, 2048) > 0
    assert call(m, k, 64) == (-2, -2)                                     # WISE_E_WORKSPACE
    assert b"workspace" in lib.wise_last_error()
    assert lib.wise_pqflat_topk(Cd.data_ptr() + 1, N, m, Ld.data_ptr(), nq, k, 0, 0, D.data_ptr(), I.data_ptr(), ws.data_ptr(), ws.numel(), 0) == -1
    assert lib.wise_pqflat_topk_pos(Cd.data_ptr(), N, m, pos.data_ptr(), N + 1, Ld.data_ptr(), nq, k, 0, 0, D.data_ptr(), I.data_ptr(), ws.data_ptr(),
                                    ws.numel(), 0) == -1               # more positions than rows
    cb = _dev(np.zeros((m, 256, 4), dtype=np.float32))
    out = torch.full((10, 64), 7.0, device="cuda")
    assert lib.wise_pqflat_decode(Cd.data_ptr(), N, pos.data_ptr(), 10, cb.data_ptr(), 64, 7, out.data_ptr(), 0) == -3      # d % m
    assert lib.wise_pqflat_decode(Cd.data_ptr(), N, pos.data_ptr(), 10, cb.data_ptr(), 64, 129, out.data_ptr(), 0) == -3
    torch.cuda.synchronize()
    assert torch.isnan(D).all() and (I == -7).all() and (out == 7.0).all()
    # nq = 0 is served and writes nothing
    assert lib.wise_pqflat_topk(Cd.data_ptr(), N, m, 0, 0, k, 0, 0, 0, 0, 0, 0, 0) == 0


# ------------------------------------------------------------------------------------------------------------------ (5) graph capture
def test_one_graph_capture_and_replay_equals_the_eager_call():
    lib = _lib.lib()
    N, d, m, nq, k = 9000, 64, 16, 5, 10
    rng = np.random.default_rng(3)
    codes = _dev(rng.integers(0, 256, (N, m)).astype(np.uint8))
    cb = _dev(rng.standard_normal((m, 256, d // m)).astype(np.float32))
    Q = _dev(rng.standard_normal((nq, d)).astype(np.float32))
    pos = _dev(np.arange(0, N, 3, dtype=np.int64))
    lut = torch.empty(nq, m, 256, dtype=torch.float32, device="cuda")
    ws = torch.empty(lib.wise_pqflat_topk_workspace_bytes(N, m, nq, k), dtype=torch.uint8, device="cuda")
    outs = [(torch.zeros(nq, k, dtype=torch.float32, device="cuda"), torch.zeros(nq, k, dtype=torch.int64, device="cuda")) for _ in range(2)]

    def run(st):
        _lib.check(lib.wise_pq_lut(Q.data_ptr(), cb.data_ptr(), nq, d, m, lut.data_ptr(), st), "wise_pq_lut")
        _lib.check(lib.wise_pqflat_topk(codes.data_ptr(), N, m, lut.data_ptr(), nq, k, 0, 100, outs[0][0].data_ptr(), outs[0][1].data_ptr(),
                                        ws.data_ptr(), ws.numel(), st), "wise_pqflat_topk")
        _lib.check(lib.wise_pqflat_topk_pos(codes.data_ptr(), N, m, pos.data_ptr(), pos.numel(), lut.data_ptr(), nq, k, 0, 100,
                                            outs[1][0].data_ptr(), outs[1][1].data_ptr(), ws.data_ptr(), ws.numel(), st), "wise_pqflat_topk_pos")

    run(_lib.stream_ptr())                                  # eager, once before the capture
    torch.cuda.synchronize()
    eager = [(D.cpu().numpy().copy(), I.cpu().numpy().copy()) for D, I in outs]
    Dr, Ir = ref.scan(codes.cpu().numpy(), None, lut.cpu().numpy(), k, id_base=100)
    assert _same(eager[0][0], Dr) and np.array_equal(eager[0][1], Ir)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(_lib.stream_ptr())
    for rep in range(2):
        lut.zero_()
        for D, I in outs:
            D.zero_()
            I.zero_()
        g.replay()
        torch.cuda.synchronize()
        for (D, I), (De, Ie) in zip(outs, eager):
            assert _same(D, De) and np.array_equal(I.cpu().numpy(), Ie), rep


# ------------------------------------------------------------------------------------------------------------------ (6) the classes
N_CLS, D_CLS, M_CLS = 5000, 64, 8


@pytest.fixture(scope="module")
def class_case():
    """Rows, ids, queries and — computed once, by the restatement alone — the trained codebooks, the codes and the tables."""
    rng = np.random.default_rng(23)
    X = (rng.standard_normal((N_CLS, D_CLS)) / np.sqrt(D_CLS)).astype(np.float32)
    ids = rng.permutation(N_CLS).astype(np.int64) + 1000
    Q = (X[:6] + 0.1 * rng.standard_normal((6, D_CLS)) / np.sqrt(D_CLS)).astype(np.float32)
    cb = ref.train_f32(X[ivfpq_ref.training_rows(N_CLS, 1234)], M_CLS, niter=10)
    codes = ref.encode_f32(X, cb)
    return dict(X=X, ids=ids, Q=Q, cb=cb, codes=codes, lut=ref.lut_f32(Q, cb))


def test_plain_class_train_add_search_reconstruct(class_case):
    from wise_amd.index.flat_pq import FlatPQIPIndex
    from wise_amd.index.selector import IDSelectorRange, SearchParameters

    c = class_case
    X, ids, Q, cb, codes, lut = c["X"], c["ids"], c["Q"], c["cb"], c["codes"], c["lut"]
    N, d, m = N_CLS, D_CLS, M_CLS
    one = FlatPQIPIndex(d, m)
    assert not one.is_trained
    for early in (lambda: one.add_with_ids(X, ids), lambda: one.add_codes_with_ids(codes, ids), lambda: one.search(Q, 3)):
        with pytest.raises(RuntimeError, match="before train"):
            early()
    with pytest.raises(ValueError, match="training vectors"):
        one.train(X[:255])
    one.train(X)
    assert one.is_trained and _same(one.codebooks, cb)                   # the trainer's bits
    one.add_with_ids(X, ids)
    with pytest.raises(RuntimeError, match="cannot change"):
        one.train(X)
    chunked = FlatPQIPIndex(d, m)
    chunked.ENCODE_BYTES = 4 * d * 300                                   # the staging: 300 rows at a time
    chunked.set_codebooks(cb)
    chunked.add_with_ids(X[:3000], ids[:3000])
    chunked.add_with_ids(_dev(X[3000:]), ids[3000:])                     # the second chunk already on the device
    loaded = FlatPQIPIndex(d, m)
    loaded.set_codebooks(cb)
    loaded.reserve(N)
    loaded.add_codes_with_ids(codes[:2000], ids[:2000])
    loaded.add_codes_with_ids(codes[2000:], ids[2000:])
    Dr, Ir = ref.scan(codes, ids, lut, 20)
    sel = IDSelectorRange(1500, 2500)
    pos = np.flatnonzero((ids >= 1500) & (ids < 2500))
    Dp, Ip = ref.scan_pos(codes, ids, lut, pos, 20)
    for idx in (one, chunked, loaded):
        Ch, ih = idx.rows_host()
        assert Ch.dtype == np.uint8 and Ch.tobytes() == codes.tobytes() and np.array_equal(ih, ids)
        assert idx.ntotal == N and idx.hbm_bytes() == N * (m + 8) + m * 256 * (d // m) * 4
        assert not hasattr(idx, "_X")                                    # no fp32 rows
        D, I = idx.search(Q, 20)
        assert _same(D, Dr) and np.array_equal(I, Ir)
        Ds, Is = idx.search(Q, 20, params=SearchParameters(sel=sel))
        assert _same(Ds, Dp) and np.array_equal(Is, Ip)
    with pytest.raises(NotImplementedError):
        one.range_search(Q, 0.5)
    want = np.array([ids[7], ids[0], 5, ids[N - 1]], dtype=np.int64)
    rec = one.reconstruct_batch(want)
    assert np.isnan(rec[2]).all() and _same(rec[[0, 1, 3]], ref.decode(codes, [7, 0, N - 1], cb))
    assert ((rec[0] - X[7]) ** 2).sum() < (X[7] ** 2).sum()              # decoded: closer to the row than nothing
    # remove_ids, then every operation: the index that received only the kept rows
    rng = np.random.default_rng(4)
    gone = np.sort(rng.permutation(N)[:777])
    keep = np.setdiff1d(np.arange(N), gone)
    assert loaded.remove_ids(ids[gone]) == 777 and loaded.remove_ids(ids[gone]) == 0
    fresh = FlatPQIPIndex(d, m)
    fresh.set_codebooks(cb)
    fresh.add_with_ids(X[keep], ids[keep])
    assert loaded.rows_host()[0].tobytes() == fresh.rows_host()[0].tobytes() == codes[keep].tobytes()
    assert np.array_equal(loaded.rows_host()[1], ids[keep]) and loaded.ntotal == N - 777
    D3, I3 = ref.scan(codes[keep], ids[keep], lut, 20)
    for idx in (loaded, fresh):
        D, I = idx.search(Q, 20)
        assert _same(D, D3) and np.array_equal(I, I3)
        assert np.isnan(idx.reconstruct_batch([ids[gone[0]]])).all()
        assert _same(idx.reconstruct_batch([ids[keep[5]]]), ref.decode(codes, [keep[5]], cb))
    loaded.add_with_ids(X[gone[:50]], ids[gone[:50]])                    # the reserved tensor is filled from the new end
    assert loaded.rows_host()[0].tobytes() == np.concatenate([codes[keep], codes[gone[:50]]]).tobytes()
    assert one.remove_ids(IDSelectorRange(0, 10 ** 9)) == N and one.ntotal == 0
    D, I = one.search(Q, 3)
    assert (I == -1).all() and (D == NEG).all()


@pytest.mark.parametrize("kind", [8, 16])
def test_refine_class_search_remove_reconstruct(class_case, kind):
    from wise_amd.index.flat_pq import FlatPQRefineIPIndex
    from wise_amd.index.selector import IDSelectorRange, SearchParameters

    c = class_case
    X, ids, Q, cb, codes, lut = c["X"], c["ids"], c["Q"], c["cb"], c["codes"], c["lut"]
    N, d, m, k = N_CLS, D_CLS, M_CLS, 10
    rows, scales = ivfpq_refine_ref.quantise(X, kind)

    def host_equal(idx, keep):
        r, s = idx.store_host()
        ok = idx.rows_host()[0].tobytes() == codes[keep].tobytes() and np.array_equal(idx.rows_host()[1], ids[keep])
        ok = ok and r.tobytes() == rows[keep].tobytes() and (s is None if kind == 16 else _same(s, scales[keep]))
        return ok and idx.ntotal == len(keep) and idx.hbm_bytes() == len(keep) * (m + 8 + (d + 4 if kind == 8 else 2 * d)) + 1024 * d

    idx = FlatPQRefineIPIndex(d, m, kind)
    assert idx.k_factor == 50
    with pytest.raises(RuntimeError, match="before train"):
        idx.add_with_ids(X, ids)
    idx.ENCODE_BYTES = 4 * d * 700
    idx.set_codebooks(cb)
    idx.add_with_ids(X[:3000], ids[:3000])                               # two chunks
    idx.add_with_ids(X[3000:], ids[3000:])
    loaded = FlatPQRefineIPIndex(d, m, kind, k_factor=7)
    loaded.set_codebooks(cb)
    loaded.reserve(N)
    loaded.add_codes_with_ids(codes[:1000], ids[:1000], rows=rows[:1000], scales=None if scales is None else scales[:1000])
    loaded.add_codes_with_ids(codes[1000:], ids[1000:], rows=rows[1000:], scales=None if scales is None else scales[1000:])
    everything = np.arange(N)
    assert host_equal(idx, everything) and host_equal(loaded, everything)
    sel = IDSelectorRange(1500, 3500)
    pos = np.flatnonzero((ids >= 1500) & (ids < 3500))
    for index, kf in ((idx, 50), (loaded, 7)):
        D, I = index.search(Q, k)
        Dr, Ir = ref.search_refine(codes, ids, lut, rows, kind, scales, Q, k, kf)
        assert _same(D, Dr) and np.array_equal(I, Ir), kf
        Ds, Is = index.search(Q, k, params=SearchParameters(sel=sel))
        Dp, Ip = ref.search_refine(codes, ids, lut, rows, kind, scales, Q, k, kf, pos=pos)
        assert _same(Ds, Dp) and np.array_equal(Is, Ip), kf
    assert (idx.search(Q, k)[1][:, 0] == ids[:6]).all()                  # re-ranked: a near copy of a row finds it
    want = np.array([ids[7], 5, ids[N - 1]], dtype=np.int64)
    rec = idx.reconstruct_batch(want)
    deq = ivfpq_refine_ref.dequantise(rows[[7, N - 1]], kind, None if scales is None else scales[[7, N - 1]])
    assert np.isnan(rec[1]).all() and _same(rec[[0, 2]], deq)
    # remove_ids compacts codes, ids, rows and scales under one plan: byte for byte the index of the kept rows
    rng = np.random.default_rng(kind)
    gone = np.sort(rng.permutation(N)[:1234])
    keep = np.setdiff1d(np.arange(N), gone)
    assert idx.remove_ids(ids[gone]) == 1234
    fresh = FlatPQRefineIPIndex(d, m, kind)
    fresh.set_codebooks(cb)
    fresh.add_with_ids(X[keep], ids[keep])
    assert host_equal(idx, keep) and host_equal(fresh, keep)
    Dr, Ir = ref.search_refine(codes[keep], ids[keep], lut, rows[keep], kind, None if scales is None else scales[keep], Q, k, 50)
    for index in (idx, fresh):
        D, I = index.search(Q, k)
        assert _same(D, Dr) and np.array_equal(I, Ir)
        assert np.isnan(index.reconstruct_batch([ids[gone[3]]])).all()
    idx.add_with_ids(X[gone[:40]], ids[gone[:40]])
    assert host_equal(idx, np.concatenate([keep, gone[:40]]))
    assert idx.remove_ids(IDSelectorRange(0, 10 ** 9)) == len(keep) + 40
    D, I = idx.search(Q, 3)
    assert (I == -1).all() and (D == NEG).all()


# ------------------------------------------------------------------------------------------------------------------ (7) the plugin
@pytest.mark.parametrize("itype", ["IndexPQ8", "IndexPQ8R8", "IndexPQ8R16"])
def test_plugin_create_load_update_and_search_within(tmp_path, itype):
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    from wise_amd.index import faiss_io
    from wise_amd.index.flat_pq import FlatPQIPIndex, FlatPQRefineIPIndex
    from wise_amd.index.search_index_factory import SearchIndexFactory

    def write_store(X, ids):
        import shutil
        shutil.rmtree(tmp_path / "features", ignore_errors=True)
        (tmp_path / "features").mkdir()
        st = FeatureStoreFactory.create_store(FeatureStoreType.NUMPY, "video", str(tmp_path / "features"))
        st.enable_write(500, 0)
        for i, v in zip(ids, X):
            st.add(int(i), v[None])
        st.close()

    kind = {"IndexPQ8": None, "IndexPQ8R8": 8, "IndexPQ8R16": 16}[itype]
    N, d, m = 1500, 512, 8
    X = ivfpq_ref.clustered_unit_rows(N, d, 40, 0.3, 9)
    ids = np.arange(N, dtype=np.int64) * 2 + 1
    write_store(X, ids)
    si = SearchIndexFactory("video", "mlfoundations/open_clip/ViT-B-32/seeded-0", {"features_dir": tmp_path / "features", "index_dir": tmp_path / "index"})
    si.create_index(itype)
    fn = si.get_index_filename(itype)
    assert fn.name == f"video-{itype}.faiss" and fn.exists()
    assert faiss_io.index_fourcc(fn) == ("IxMp" if kind is None else "WiFR")
    assert kind is not None or faiss_io.index_fourcc(fn, inner=True) == "IxPq"
    assert faiss_io.index_ntotal(fn) == N
    f = faiss_io.read_index(fn)
    cb = f["codebooks"]
    assert cb.shape == (m, 256, d // m) and f["codes"].shape == (N, m) and np.array_equal(f["ids"], ids)
    assert kind is None or (f["kind"] == kind and f["k_factor"] == 50)

    def built_from(Xs, ids_s):
        """the file of an index built from these rows with the codebooks of the file under test"""
        idx = FlatPQIPIndex(d, m) if kind is None else FlatPQRefineIPIndex(d, m, kind)
        idx.set_codebooks(cb)
        idx.add_with_ids(Xs, ids_s)
        want = tmp_path / "want.faiss"
        faiss_io.write_index(want, idx.state_host())
        return hashlib.sha256(want.read_bytes()).hexdigest()

    assert hashlib.sha256(fn.read_bytes()).hexdigest() == built_from(X, ids)
    assert si.load_index(itype) is True and si.is_index_loaded()
    index = si.index
    assert type(index) is (FlatPQIPIndex if kind is None else FlatPQRefineIPIndex) and index.m == m and index.ntotal == N
    D, I = index.search(X[:8], 5)
    assert (np.diff(D, axis=1) <= 0).all() and (kind is None or (I[:, 0] == ids[:8]).all())      # re-ranked: a row finds itself
    dist, got = si.search("video", "dog", topk=5)
    assert dist.shape == (5,) and got.shape == (5,) and (got >= 1).all()
    inside = ids[100:140]
    dist, got = si.search("video", "dog", topk=5, within=inside)
    assert np.isin(got, inside).all() and (np.diff(dist) <= 0).all()
    # update_index: 100 vectors leave, 60 arrive at the end of the store; the codebooks and k_factor stay
    rng = np.random.default_rng(31)
    gone = np.sort(rng.permutation(N)[:100])
    stay = np.setdiff1d(np.arange(N), gone)
    newX = ivfpq_ref.clustered_unit_rows(60, d, 40, 0.3, 10)
    new_ids = np.arange(60, dtype=np.int64) + 10 ** 6
    X2, ids2 = np.concatenate([X[stay], newX]), np.concatenate([ids[stay], new_ids])
    write_store(X2, ids2)
    assert si.update_index(itype) == (60, 100)
    assert hashlib.sha256(fn.read_bytes()).hexdigest() == built_from(X2, ids2)
    assert _same(faiss_io.read_index(fn)["codebooks"], cb)
    assert si.update_index(itype) == (0, 0)

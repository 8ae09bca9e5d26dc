"""-m gpu: IndexIVFPQ<m> and its R8 / R16 forms sharded across ranks (wise_amd/index/sharded.py ShardedIVFPQIPIndex,
ShardedIVFPQRefineIPIndex).

(1) One process, emulated ranks: the list-major codes cut into W clipped slices, wise_ivfpq_scan_local on every slice, then
    wise_topk_merge of the W answers in rank order, gives the bits of wise_ivfpq_scan over the whole array — with ids and with
    global positions, ties across rank boundaries, ranks without rows and padding included; one slice equals the float32
    restatement tests/ivfpq_ref.py.
(2) Both stores: merge of the local candidates, wise_ivf_refine_local per slice, merge == wise_ivf_refine on the whole store.
(3) The index classes, the refusals, graph capture.
(4) The plugin path on RCCL at world size 1, in a child process with its own time limit (tests/sharded_ivfpq_nccl_worker.py)."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import ivfpq_ref
import ivfpq_refine_ref as rr
from wise_amd import _lib
from wise_amd.index.ivf_pq import IVFPQIPIndex, IVFPQRefineIPIndex
from wise_amd.index.sharded import merge_device, shard_range

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
WORLDS = (2, 3, 8)


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32) if a.dtype == torch.float32 else a,
                                              b.contiguous().view(torch.int32) if b.dtype == torch.float32 else b)


def _lists(N, m, nlist, seed):
    """Random codes in list-major order, some lists empty; at every rank boundary of W = 2, 3, 8 that falls inside a list the
    rows on its two sides carry equal codes (equal scores whatever the query).  -> (codes, ids, off, boundaries duplicated)."""
    rng = np.random.default_rng(seed)
    w = rng.random(nlist) * (rng.random(nlist) > 0.1)
    sizes = rng.multinomial(N, w / w.sum()).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    codes = rng.integers(0, 256, size=(N, m), dtype=np.uint8)
    lists = np.repeat(np.arange(nlist), sizes)
    dups = []
    for W in WORLDS:
        for r in range(1, W):
            b = shard_range(N, r, W)[0]
            if 0 < b < N and lists[b] == lists[b - 1]:
                codes[b] = codes[b - 1]
                dups.append(b)
    ids = rng.permutation(4 * N)[:N].astype(np.int64) + 5
    return codes, ids, off, sorted(set(dups))


def _tables(nq, m, nprobe, nlist, seed, favour=None, codes=None):
    """lut [nq,m,256], probes [nq,nprobe] (distinct lists, -1 padding past nlist), bias.  favour: rows whose codes get the
    largest table entries of query q, so that row (and its duplicate) leads that query's answer."""
    rng = np.random.default_rng(seed)
    lut = rng.standard_normal((nq, m, 256)).astype(np.float32)
    if favour is not None:
        for q, row in enumerate(favour[:nq]):
            lut[q, np.arange(m), codes[row]] = 9.0
    probes = np.full((nq, nprobe), -1, dtype=np.int64)
    for q in range(nq):
        p = rng.permutation(nlist)[:nprobe]
        probes[q, :len(p)] = p
    bias = rng.standard_normal((nq, nprobe)).astype(np.float32)
    return lut, probes, bias


def _scan_full(codes, off, ids, lut, probes, bias, k):
    lib = _lib.lib()
    nq, nprobe = probes.shape
    N, m = codes.shape
    D = torch.empty(nq, k, dtype=torch.float32, device="cuda")
    I = torch.empty(nq, k, dtype=torch.int64, device="cuda")
    need = lib.wise_ivfpq_scan_workspace_bytes(nq, nprobe, k, m)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _lib.check(lib.wise_ivfpq_scan(codes.data_ptr(), N, m, off.data_ptr(), off.numel() - 1, _lib.ptr(ids), lut.data_ptr(), nq,
                                   probes.data_ptr(), bias.data_ptr(), nprobe, k, D.data_ptr(), I.data_ptr(), ws.data_ptr(),
                                   ws.numel(), _lib.stream_ptr()), "wise_ivfpq_scan")
    return D, I


def _scan_local(codes, off, ids, lut, probes, bias, k, pos_base):
    lib = _lib.lib()
    nq, nprobe = probes.shape
    N, m = codes.shape
    D = torch.empty(nq, k, dtype=torch.float32, device="cuda")
    I = torch.empty(nq, k, dtype=torch.int64, device="cuda")
    cnt = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
    need = lib.wise_ivfpq_scan_local_workspace_bytes(nq, nprobe, k, m)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _lib.check(lib.wise_ivfpq_scan_local(codes.data_ptr(), N, m, off.data_ptr(), off.numel() - 1, _lib.ptr(ids), lut.data_ptr(), nq,
                                         probes.data_ptr(), bias.data_ptr(), nprobe, k, pos_base, D.data_ptr(), I.data_ptr(),
                                         cnt.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "wise_ivfpq_scan_local")
    return D, I, cnt


def _slice_codes(codes, lo, hi):
    m = codes.shape[1]
    return _dev(codes[lo:hi]).reshape(hi - lo, m)         # a fresh allocation: 16-byte aligned whatever lo is


def _emulate(codes, ids, off, lut, probes, bias, k, worlds, with_ids):
    """Whole scan vs W emulated ranks; -> the whole answer (numpy)."""
    N, m = codes.shape
    cd, idd, offd = _dev(codes), _dev(ids), _dev(off)
    ld, pd, bd = _dev(lut), _dev(probes), _dev(bias)
    Df, If = _scan_full(cd, offd, idd if with_ids else None, ld, pd, bd, k)
    for W in worlds:
        Ds, Is = [], []
        for r in range(W):
            lo, hi = shard_range(N, r, W)
            loff = np.clip(off - lo, 0, hi - lo)
            D, I, cnt = _scan_local(_slice_codes(codes, lo, hi), _dev(loff), _dev(ids[lo:hi]) if with_ids else None, ld, pd, bd, k, lo)
            want = np.where(probes >= 0, (loff[1:] > loff[:-1])[probes.clip(0)], False).sum(axis=1)
            assert np.array_equal(cnt.cpu().numpy(), want), (W, r)
            if hi == lo:
                assert (I == -1).all()
            Ds.append(D)
            Is.append(I)
        Dm, Im = merge_device(torch.stack(Ds), torch.stack(Is), k)
        assert _same_bits(Dm, Df) and _same_bits(Im, If), f"W={W} nq={probes.shape[0]} nprobe={probes.shape[1]} k={k} ids={with_ids}"
    return Df.cpu().numpy(), If.cpu().numpy()


@pytest.mark.parametrize("m", [8, 64, 128])
def test_emulated_ranks_give_the_bits_of_the_whole_scan(m):
    N, nlist = 40000, 1100
    codes, ids, off, dups = _lists(N, m, nlist, seed=m)
    assert len(dups) >= 4
    combos = [(nq, nprobe, k) for nq in (1, 3, 256) for nprobe in (1, 32, 1024) for k in (10, 100, 1000, 2048)]
    combos = combos[(m // 8) % 3::3]                       # thinned (3 is coprime to the 4 values of k): every value of nq, nprobe and k occurs for every m
    assert {c[0] for c in combos} == {1, 3, 256} and {c[1] for c in combos} == {1, 32, 1024} and {c[2] for c in combos} == {10, 100, 1000, 2048}
    lists_of = ivfpq_ref.list_of_rows(off)
    tie_checked = 0
    for n, (nq, nprobe, k) in enumerate(combos):
        lut, probes, bias = _tables(nq, m, nprobe, nlist, seed=1000 * m + n, favour=dups, codes=codes)
        for q in range(min(nq, len(dups))):               # the favoured pair's list is probed first
            l = lists_of[dups[q]]
            if l not in probes[q]:
                probes[q, 0] = l
        with_ids = n % 2 == 0
        Df, If = _emulate(codes, ids, off, lut, probes, bias, k, WORLDS, with_ids)
        for q in range(min(nq, len(dups))):               # two rows with equal codes on the two sides of a rank boundary
            b = dups[q]
            if k >= 2 and Df[q, 0] == Df[q, 1]:
                pair = [ids[b - 1], ids[b]] if with_ids else [b - 1, b]
                if list(If[q, :2]) == pair:
                    tie_checked += 1
        if nprobe == 1 and k >= 1000:
            assert (If == -1).any()                        # fewer than k probed rows: padding
    assert tie_checked > 0


@pytest.mark.parametrize("d,m", [(512, 64), (768, 8)])
def test_one_slice_equals_the_float32_restatement(d, m):
    N, nlist, nq, nprobe, k = 6000, 150, 3, 32, 100
    codes, ids, off, _ = _lists(N, m, nlist, seed=d)
    lut, probes, bias = _tables(nq, m, nprobe, nlist, seed=d + 1)
    lo, hi = shard_range(N, 1, 3)
    loff = np.clip(off - lo, 0, hi - lo)
    D, I, _ = _scan_local(_slice_codes(codes, lo, hi), _dev(loff), _dev(ids[lo:hi]), _dev(lut), _dev(probes), _dev(bias), k, lo)
    Dr, Ir = ivfpq_ref.scan(codes[lo:hi], loff, ids[lo:hi], lut, probes, bias, k)
    assert np.array_equal(D.cpu().numpy().view(np.int32), Dr.view(np.int32)) and np.array_equal(I.cpu().numpy(), Ir)
    D, I, _ = _scan_local(_slice_codes(codes, lo, hi), _dev(loff), None, _dev(lut), _dev(probes), _dev(bias), k, lo)
    Dr, Ir = ivfpq_ref.scan(codes[lo:hi], loff, None, lut, probes, bias, k)
    assert np.array_equal(D.cpu().numpy().view(np.int32), Dr.view(np.int32))
    assert np.array_equal(I.cpu().numpy(), np.where(Ir >= 0, Ir + lo, -1))        # positions in the whole array


def test_ranks_without_rows_and_padding():
    m, nlist = 64, 6
    codes, ids, off, _ = _lists(5, m, nlist, seed=9)
    lut, probes, bias = _tables(3, m, 6, nlist, seed=4)
    for with_ids in (True, False):
        Df, If = _emulate(codes, ids, off, lut, probes, bias, 10, WORLDS, with_ids)      # W = 8 > 5 rows: three ranks hold nothing
        assert (If[:, 5:] == -1).all() and (If[:, :5] >= 0).all()


# ------------------------------------------------------------------------------------------------------------------ refine
def _refine(rows, scales, ids, Q, cand, k, kind, pos_base=None):
    lib = _lib.lib()
    nq, kc = cand.shape
    N, d = rows.shape
    D = torch.empty(nq, k, dtype=torch.float32, device="cuda")
    I = torch.empty(nq, k, dtype=torch.int64, device="cuda")
    head = (_lib.ptr(rows), kind, _lib.ptr(scales), N, d, _lib.ptr(ids), Q.data_ptr(), nq, cand.data_ptr(), kc, k)
    if pos_base is None:
        _lib.check(lib.wise_ivf_refine(*head, D.data_ptr(), I.data_ptr(), _lib.stream_ptr()), "wise_ivf_refine")
    else:
        _lib.check(lib.wise_ivf_refine_local(*head, pos_base, D.data_ptr(), I.data_ptr(), _lib.stream_ptr()), "wise_ivf_refine_local")
    return D, I


def _store(N, d, kind, seed):
    X = _unit(np.random.default_rng(seed).standard_normal((N, d)))
    for W in WORLDS:                                        # equal rows on the two sides of every rank boundary
        for r in range(1, W):
            b = shard_range(N, r, W)[0]
            X[b] = X[b - 1]
    rows, scales = rr.quantise(X, kind)
    return X, (rows if kind == 8 else rows.view(np.int16)), scales


@pytest.mark.parametrize("kind,d", [(8, 512), (16, 768), (8, 768), (16, 512)])
def test_two_phase_emulation_equals_the_whole_refine(kind, d):
    N, m, nlist, nq, nprobe = 20000, 64, 400, 5, 64
    codes, ids, off, _ = _lists(N, m, nlist, seed=kind + d)
    X, rows, scales = _store(N, d, kind, seed=d)
    Q = _unit(np.random.default_rng(5).standard_normal((nq, d)))
    Q[0] = X[shard_range(N, 1, 2)[0]]                      # its two equal rows sit on two ranks for W = 2
    lut, probes, bias = _tables(nq, m, nprobe, nlist, seed=kind)
    cd, idd, offd, ld, pd, bd, Qd = _dev(codes), _dev(ids), _dev(off), _dev(lut), _dev(probes), _dev(bias), _dev(Q)
    rd, sd = _dev(rows), (None if scales is None else _dev(scales))
    for kc, k in [(1, 1), (100, 10), (2048, 100), (2048, 2048)]:
        _, cand = _scan_full(cd, offd, None, ld, pd, bd, kc)
        if kc == 100:                                       # holes, a duplicate, and the pair of equal rows
            cand = cand.clone()
            cand[:, 3] = -1
            cand[:, 7] = N + 11
            cand[:, 9] = cand[:, 8]
            b = shard_range(N, 1, 2)[0]
            cand[0][(cand[0] == b) | (cand[0] == b - 1)] = -1
            cand[0, 0], cand[0, 1] = b, b - 1
        Dw, Iw = _refine(rd, sd, idd, Qd, cand, k, kind)
        Dp, Ip = _refine(rd, sd, None, Qd, cand, k, kind)
        # pos_base = 0 over the whole store is wise_ivf_refine
        D0, I0 = _refine(rd, sd, idd, Qd, cand, k, kind, pos_base=0)
        assert _same_bits(D0, Dw) and _same_bits(I0, Iw)
        for W in WORLDS:
            cDs, cIs, sl = [], [], []
            for r in range(W):
                lo, hi = shard_range(N, r, W)
                loff = np.clip(off - lo, 0, hi - lo)
                D, I, _ = _scan_local(_slice_codes(codes, lo, hi), _dev(loff), None, ld, pd, bd, kc, lo)
                cDs.append(D)
                cIs.append(I)
                sl.append((lo, hi))
            _, gc = merge_device(torch.stack(cDs), torch.stack(cIs), kc)
            if kc != 100:
                assert _same_bits(gc, cand), (W, kc)        # phase 1: the candidates of the one-GPU scan
            else:
                gc = cand
            for use_ids, (Dwant, Iwant) in ((True, (Dw, Iw)), (False, (Dp, Ip))):
                Ds, Is = [], []
                for lo, hi in sl:
                    D, I = _refine(_dev(rows[lo:hi]).reshape(hi - lo, d), None if scales is None else _dev(scales[lo:hi]),
                                   _dev(ids[lo:hi]) if use_ids else None, Qd, gc, k, kind, pos_base=lo)
                    Ds.append(D)
                    Is.append(I)
                Dm, Im = merge_device(torch.stack(Ds), torch.stack(Is), k)
                assert _same_bits(Dm, Dwant) and _same_bits(Im, Iwant), (W, kc, k, use_ids)
        if kc == 100:
            b = shard_range(N, 1, 2)[0]
            Dh, Ih = Dp.cpu().numpy(), Ip.cpu().numpy()
            assert Dh[0, 0] == Dh[0, 1] and list(Ih[0, :2]) == [b - 1, b]      # a tie across the boundary, lower position first
            Dr, Ir = rr.refine(rows if kind == 8 else rows.view(np.uint16), kind, scales, None, Q, cand.cpu().numpy(), k)
            assert np.array_equal(Dh.view(np.int32), Dr.view(np.int32)) and np.array_equal(Ih, Ir)


def test_refine_local_under_graph_capture():
    N, d, nq, kc, k, kind, lo = 3000, 512, 4, 100, 10, 8, 1000
    X, rows, scales = _store(N, d, kind, seed=3)
    rng = np.random.default_rng(2)
    Q, cand = _dev(_unit(rng.standard_normal((nq, d)))), _dev(rng.integers(0, N, size=(nq, kc)).astype(np.int64))
    rd, sd, idd = _dev(rows[lo:2000]), _dev(scales[lo:2000]), _dev(np.arange(1000, dtype=np.int64) + 77)
    De, Ie = _refine(rd, sd, idd, Q, cand, k, kind, pos_base=lo)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D, I = _refine(rd, sd, idd, Q, cand, k, kind, pos_base=lo)
    D.zero_()
    I.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert _same_bits(D, De) and _same_bits(I, Ie) and int((Ie >= 0).sum()) > 0


def test_unsupported_shapes_are_refused_with_a_message():
    lib = _lib.lib()
    assert lib.wise_ivfpq_scan_local_workspace_bytes(4, 2049, 10, 64) == 0
    assert lib.wise_ivfpq_scan_local_workspace_bytes(4, 16, 2049, 64) == 0
    assert lib.wise_ivfpq_scan_local_workspace_bytes(4, 16, 10, 129) == 0
    assert lib.wise_ivfpq_scan_local_workspace_bytes(65536, 16, 10, 64) == 0
    assert lib.wise_ivfpq_scan_local(0, 0, 129, 0, 1, 0, 0, 1, 0, 0, 1, 10, 0, 0, 0, 0, 0, 0, 0) == -3
    assert b"m <= 128" in lib.wise_last_error()
    assert lib.wise_ivf_refine_local(0, 8, 0, 0, 500, 0, 0, 1, 0, 10, 10, 0, 0, 0, 0) == -3
    assert b"ivf_refine_local" in lib.wise_last_error() and b"d %" in lib.wise_last_error()
    assert lib.wise_ivf_refine_local(0, 16, 0, 0, 512, 0, 0, 1, 0, 2049, 10, 0, 0, 0, 0) == -3
    assert b"kc=2049" in lib.wise_last_error()
    assert lib.wise_ivf_refine_local(0, 16, 0, 0, 512, 0, 0, 1, 0, 10, 10, -1, 0, 0, 0) == -1
    assert b"pos_base" in lib.wise_last_error()


# ------------------------------------------------------------------------------------------------------------------ index level
def _trained(cls, d, nlist, m, X, ids, *a):
    idx = cls(d, nlist, m, *a)
    idx.train(X[:8000])
    idx.add_with_ids(X, ids)
    return idx


@pytest.mark.parametrize("kind", [None, 8, 16])
def test_index_slices_and_merge_equal_the_whole_index(kind):
    d, m, N, nlist, k, W, nq = 512, 64, 20000, 128, 20, 4, 5
    X = ivfpq_ref.clustered_unit_rows(N, d, 64, 0.35, seed=11)
    ids = np.random.default_rng(1).permutation(3 * N)[:N].astype(np.int64)
    full = _trained(IVFPQIPIndex, d, nlist, m, X, ids) if kind is None else _trained(IVFPQRefineIPIndex, d, nlist, m, X, ids, kind, 20)
    full.nprobe = 24
    c, cb, codes, ids_s, off = full.lists_host()
    Q = _dev(_unit(X[:nq] + 0.05 * np.random.default_rng(2).standard_normal((nq, d)).astype(np.float32)))
    Dw, Iw = full.search_device(Q, k)
    locs = []
    for r in range(W):
        lo, hi = shard_range(N, r, W)
        loff = torch.from_numpy(np.clip(off - lo, 0, hi - lo))
        if kind is None:
            loc = IVFPQIPIndex(d, nlist, m)
            loc.adopt_lists(torch.from_numpy(codes[lo:hi]), torch.from_numpy(ids_s[lo:hi]), loff, pos_base=lo)
        else:
            rows, scales = full.store_host()
            loc = IVFPQRefineIPIndex(d, nlist, m, kind, k_factor=20)
            loc.adopt_lists(torch.from_numpy(codes[lo:hi]), torch.from_numpy(ids_s[lo:hi]), loff,
                            torch.from_numpy(rows[lo:hi] if kind == 8 else rows[lo:hi].view(np.int16)),
                            None if scales is None else torch.from_numpy(scales[lo:hi]), pos_base=lo)
        loc.set_centroids(c)
        loc.set_codebooks(cb)
        loc.nprobe = 24
        assert loc.pos_base == lo
        locs.append(loc)
    if kind is None:
        cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
        parts = [loc.search_local_device(Q, k, probe_count=cnt) for loc in locs]
        assert 0 < int(cnt.max()) <= 24
        Dm, Im = merge_device(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]), k)
        # positions=True: the positions of the whole array
        Dp, Ip = merge_device(*map(torch.stack, zip(*[loc.search_local_device(Q, k, positions=True) for loc in locs])), k)
        assert _same_bits(Dp, Dw) and torch.equal(_dev(ids_s)[Ip], Iw)
    else:
        kc = full.candidates(k)
        cands = [loc.candidates_local_device(Q, kc) for loc in locs]
        _, gc = merge_device(torch.stack([p[0] for p in cands]), torch.stack([p[1] for p in cands]), kc)
        parts = [loc.refine_local_device(Q, gc, k) for loc in locs]
        Dm, Im = merge_device(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]), k)
        with pytest.raises(NotImplementedError):
            locs[0].search_local_device(Q, k)
    assert _same_bits(Dm, Dw) and _same_bits(Im, Iw) and int((Iw >= 0).sum()) == nq * k


def test_sharded_refine_wrapper_refuses_more_ranks_than_one_merge_takes(monkeypatch):
    from wise_amd.index import sharded

    loc = IVFPQRefineIPIndex(512, 4, 64, 8, k_factor=50)
    w = sharded.ShardedIVFPQRefineIPIndex(loc)
    monkeypatch.setattr(sharded.ShardedFlatIPIndex, "world", property(lambda self: 33))
    monkeypatch.setattr(sharded.ShardedFlatIPIndex, "_exchanges", lambda self: True)
    with pytest.raises(ValueError, match="33 ranks x 2048 candidates"):
        w.search_device(torch.zeros(1, 512, device="cuda"), 100)


# ------------------------------------------------------------------------------------------------------------------ RCCL
def test_sharded_ivfpq_plugin_over_rccl_world1(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "sharded_ivfpq_nccl_worker.py"), str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert res["ok"], json.dumps(res)
    nq, k = 3, 10
    assert res["exchange_bytes"]["IndexIVFPQ16"] == 16 * nq * k                      # one exchange of (score, id) planes
    for t in ("IndexIVFPQ16R8", "IndexIVFPQ16R16"):
        assert res["exchange_bytes"][t] == 16 * nq * (res["candidates"] + k)         # candidates, then re-ranked answers
    assert res["candidates"] == 500

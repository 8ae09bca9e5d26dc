"""-m gpu: IndexIVFFlat sharded across ranks (wise_amd/index/sharded.py ShardedIVFFlatIPIndex).

(1) One process, emulated ranks: an index cut into W clipped slices of its list-major array, wise_ivf_scan_local_f32 on
    every slice, then wise_topk_merge of the W answers in rank order, gives the same bits as wise_ivf_scan_f32 over the
    whole index — ties across rank boundaries, ranks without rows and padding included.
(2) The plugin path on RCCL at world size 1 (create_index -> part file -> load_index -> collective search), in a child
    process with its own time limit (tests/sharded_ivf_nccl_worker.py)."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import ivf_ref
from wise_amd import _lib
from wise_amd.index.ivf_flat import IVFFlatIPIndex
from wise_amd.index.sharded import merge_device, shard_range

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _index(N, d, nlist, seed):
    """A list-major index whose rows lie near their list's centroid; some lists empty; equal rows on both sides of
    every rank boundary of W = 2, 3, 8 and at the two ends of the array."""
    rng = np.random.default_rng(seed)
    c = _unit(rng.standard_normal((nlist, d)))
    w = rng.random(nlist) * (rng.random(nlist) > 0.1)
    sizes = rng.multinomial(N, w / w.sum()).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    lists = np.repeat(np.arange(nlist), sizes)
    X = _unit(c[lists] + 0.35 * rng.standard_normal((N, d)).astype(np.float32))
    dups = []
    for W in (2, 3, 8):
        for r in range(1, W):
            b = shard_range(N, r, W)[0]
            if 0 < b < N:
                X[b] = X[b - 1]
                dups.append(b)
    if N > 1:
        X[N - 1] = X[0]
        dups.append(0)
    ids = rng.permutation(4 * N)[:N].astype(np.int64) + 5
    return c, X, ids, off, dups


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _scan_full(X, ids, off, Q, probes, k):
    lib = _lib.lib()
    nq, nprobe = probes.shape
    D = torch.empty(nq, k, dtype=torch.float32, device="cuda")
    I = torch.empty(nq, k, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.wise_ivf_scan_workspace_bytes(nq, nprobe, k), dtype=torch.uint8, device="cuda")
    _lib.check(lib.wise_ivf_scan_f32(X.data_ptr(), X.shape[0], X.shape[1], off.data_ptr(), off.numel() - 1, ids.data_ptr(),
                                     Q.data_ptr(), nq, probes.data_ptr(), nprobe, k, D.data_ptr(), I.data_ptr(),
                                     ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "wise_ivf_scan_f32")
    return D, I


def _scan_local(X, ids, off, Q, probes, k):
    lib = _lib.lib()
    nq, nprobe = probes.shape
    D = torch.empty(nq, k, dtype=torch.float32, device="cuda")
    I = torch.empty(nq, k, dtype=torch.int64, device="cuda")
    cnt = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
    need = lib.wise_ivf_scan_local_workspace_bytes(nq, nprobe, k)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _lib.check(lib.wise_ivf_scan_local_f32(X.data_ptr(), X.shape[0], X.shape[1], off.data_ptr(), off.numel() - 1,
                                           ids.data_ptr(), Q.data_ptr(), nq, probes.data_ptr(), nprobe, k, D.data_ptr(),
                                           I.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               "wise_ivf_scan_local_f32")
    return D, I, cnt


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32) if a.dtype == torch.float32 else a,
                                              b.contiguous().view(torch.int32) if b.dtype == torch.float32 else b)


def _emulate(c, X, ids, off, Q, nprobe, k, worlds):
    """Full scan vs. W emulated ranks for every W; returns the full answer (numpy) for further checks."""
    N, d = X.shape
    nlist = c.shape[0]
    full = IVFFlatIPIndex(d, nlist)
    full.set_centroids(c)
    full.adopt_lists(_dev(X), _dev(ids), _dev(off))
    Qd = _dev(Q)
    probes = full.probes_device(Qd, nprobe).contiguous()
    Xd, idd, offd = full._lists.data, full._lists.ids, full._lists.list_off
    Df, If = _scan_full(Xd, idd, offd, Qd, probes, k)
    pr = probes.cpu().numpy()
    for W in worlds:
        Ds, Is = [], []
        for r in range(W):
            lo, hi = shard_range(N, r, W)
            loff = np.clip(off - lo, 0, hi - lo)
            D, I, cnt = _scan_local(_dev(X[lo:hi]).reshape(hi - lo, d), _dev(ids[lo:hi]), _dev(loff), Qd, probes, k)
            want = np.where(pr >= 0, (loff[1:] > loff[:-1])[pr.clip(0)], False).sum(axis=1)
            assert np.array_equal(cnt.cpu().numpy(), want), (W, r)
            if hi == lo:
                assert (I == -1).all()
            Ds.append(D)
            Is.append(I)
        Dm, Im = merge_device(torch.stack(Ds), torch.stack(Is), k)
        assert _same_bits(Dm, Df) and _same_bits(Im, If), f"W={W} nq={len(Q)} nprobe={nprobe} k={k}: bits differ"
    return Df.cpu().numpy(), If.cpu().numpy(), pr, Xd, idd, offd


@pytest.mark.parametrize("d", [768, 512])
def test_emulated_ranks_give_the_bits_of_the_whole_index(d):
    N, nlist = 40000, 1100
    c, X, ids, off, dups = _index(N, d, nlist, seed=d)
    rng = np.random.default_rng(3)
    Qall = _unit(rng.standard_normal((256, d)))
    Qall[:len(dups)] = X[dups]                      # the duplicated rows are the queries' best: ties decide the order
    combos = [(nq, nprobe, k) for nq in (1, 3, 256) for nprobe in (1, 32, 1024) for k in (10, 100, 1000)]
    if d == 512:
        combos = combos[::2]
    tie_checked = 0
    for nq, nprobe, k in combos:
        Q = Qall[:nq]
        Df, If, pr, *_ = _emulate(c, X, ids, off, Q, nprobe, k, (2, 3, 8))
        for q in range(nq):                         # a query equal to a duplicated row: its two copies lead, lower row first
            if q < len(dups) and If[q, 1] >= 0 and Df[q, 0] == Df[q, 1]:
                b = dups[q]
                pair = [ids[b - 1], ids[b]] if b > 0 else [ids[0], ids[N - 1]]
                if list(If[q, :2]) == pair:
                    tie_checked += 1
        if nprobe == 1 and k == 1000:
            assert (If == -1).any()                 # fewer than k probed rows: padding
    assert tie_checked > 0


def test_ranks_without_rows_and_padding():
    d, nlist = 512, 6
    c, X, ids, off, _ = _index(5, d, nlist, seed=9)
    Q = _unit(np.random.default_rng(4).standard_normal((3, d)))
    Q[0] = X[2]
    Df, If, *_ = _emulate(c, X, ids, off, Q, 6, 10, (2, 3, 8))      # W = 8 > 5 rows: three ranks hold nothing
    assert (If[:, 5:] == -1).all() and (If[:, :5] >= 0).all()


def test_ivf_scan_unchanged_and_local_index_method():
    d, N, nlist, k = 768, 30000, 500, 50
    c, X, ids, off, _ = _index(N, d, nlist, seed=21)
    Q = _unit(np.random.default_rng(8).standard_normal((5, d)))
    Df, If, pr, Xd, idd, offd = _emulate(c, X, ids, off, Q, 40, k, (3,))
    Do, Io = ivf_ref.ivf_search(X, ids, off, Q, pr, k)                # wise_ivf_scan_f32 still answers as before
    assert np.allclose(Df, Do, atol=2e-5)
    gap = np.ones_like(Io, dtype=bool)
    gap[:, 1:] &= (Do[:, :-1] - Do[:, 1:]) > 2e-5
    gap[:, :-1] &= (Do[:, :-1] - Do[:, 1:]) > 2e-5
    assert np.array_equal(If[gap], Io[gap])
    # IVFFlatIPIndex.search_local_device on every slice + merge == search_device on the whole index
    full = IVFFlatIPIndex(d, nlist)
    full.set_centroids(c)
    full.adopt_lists(_dev(X), _dev(ids), _dev(off))
    full.nprobe = 40
    Dw, Iw = full.search_device(_dev(Q), k)
    Ds, Is = [], []
    for r in range(4):
        lo, hi = shard_range(N, r, 4)
        loc = IVFFlatIPIndex(d, nlist)
        loc.set_centroids(c)
        loc.adopt_lists(torch.from_numpy(X[lo:hi]), torch.from_numpy(ids[lo:hi]), torch.from_numpy(np.clip(off - lo, 0, hi - lo)))
        loc.nprobe = 40
        cnt = torch.zeros(5, dtype=torch.int32, device="cuda")
        D, I = loc.search_local_device(_dev(Q), k, probe_count=cnt)
        assert int(cnt.sum()) > 0 and int(cnt.max()) <= 40
        Ds.append(D)
        Is.append(I)
    Dm, Im = merge_device(torch.stack(Ds), torch.stack(Is), k)
    assert _same_bits(Dm, Dw) and _same_bits(Im, Iw)


def test_local_scan_refuses_what_it_does_not_serve():
    lib = _lib.lib()
    assert lib.wise_ivf_scan_local_workspace_bytes(4, 2049, 10) == 0
    assert lib.wise_ivf_scan_local_workspace_bytes(4, 16, 2049) == 0
    assert lib.wise_ivf_scan_local_f32(0, 0, 510, 0, 1, 0, 0, 1, 0, 1, 10, 0, 0, 0, 0, 0, 0) == -1
    assert b"multiple of 4" in lib.wise_last_error()


def test_sharded_ivf_plugin_over_rccl_world1(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "sharded_ivf_nccl_worker.py"), str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert res["ok"], json.dumps(res)
    assert res["exchange_bytes"] == 2 * 3 * 100 * 8          # the last search: nq = 3, k = 100, (score, id) planes of int64

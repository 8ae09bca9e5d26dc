"""-m gpu: IndexIVFFlatL2 sharded across ranks (wise_amd/index/sharded.py: ShardedIVFFlatIPIndex around IVFFlatL2Index slices).

(1) One process, emulated ranks: the list-major rows cut into W clipped slices, wise_ivfl2_scan_local on every slice, then
    wise_topk_merge of the W NEGATED answers in rank order, negated back, gives the bits of wise_ivfl2_scan over the whole array —
    with ids and with global positions, ties on both sides of a boundary inside a list, ranks without rows and padding included;
    probe_count against the host's count.
(2) Graph capture of the local scan, the refusals.
(3) The index class: slices of one IVFFlatL2Index, merged, against the whole index; the wrapper outside a process group.
(4) The plugin path on RCCL at world size 1, in a child process with its own time limit (tests/sharded_ivf_l2_nccl_worker.py)."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import ivf_l2_ref as ref
from wise_amd import _lib
from wise_amd.index.sharded import merge_device, shard_range

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
WORLDS = (1, 3, 8)
WISE_E_INVALID = -1
PAD = ref.PAD


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32) if a.dtype == torch.float32 else a,
                                              b.contiguous().view(torch.int32) if b.dtype == torch.float32 else b)


def _lists(N, d, nlist, seed):
    """Rows of lengths spread over 4x in list-major order in lists of uneven length, some empty.  -> (X, ids, off)"""
    rng = np.random.default_rng(seed)
    w = rng.random(nlist) * (rng.random(nlist) > 0.15)
    sizes = rng.multinomial(N, w / w.sum()).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ids = rng.permutation(4 * N)[:N].astype(np.int64) + 5
    return ref.long_rows(N, d, seed + 77), ids, off


def _queries(nq, d, nprobe, nlist, seed):
    """Q [nq,d], probes [nq,nprobe] (distinct lists, -1 padding past nlist)"""
    rng = np.random.default_rng(seed)
    probes = np.full((nq, nprobe), -1, dtype=np.int64)
    for q in range(nq):
        p = rng.permutation(nlist)[:nprobe]
        probes[q, :len(p)] = p
    return ref.long_rows(nq, d, seed + 1), probes


def _scan_full(X, off, ids, Q, probes, k):
    lib = _lib.lib()
    nq, nprobe = probes.shape
    N, d = X.shape
    D = torch.empty(nq, k, dtype=torch.float32, device="cuda")
    I = torch.empty(nq, k, dtype=torch.int64, device="cuda")
    need = lib.wise_ivfl2_scan_workspace_bytes(nq, nprobe, k)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _lib.check(lib.wise_ivfl2_scan(X.data_ptr(), N, d, off.data_ptr(), off.numel() - 1, _lib.ptr(ids), Q.data_ptr(), nq, probes.data_ptr(),
                                   nprobe, k, D.data_ptr(), I.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "wise_ivfl2_scan")
    return D, I


def _scan_local_raw(X, N, d, off, ids, Q, probes, k, pos_base, ws_bytes=None):
    """-> (return code, D, I, probe_count); X may be None when N == 0"""
    lib = _lib.lib()
    nq, nprobe = probes.shape
    D = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    I = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    cnt = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
    need = lib.wise_ivfl2_scan_local_workspace_bytes(nq, nprobe, k)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
    rc = lib.wise_ivfl2_scan_local(_lib.ptr(X), N, d, off.data_ptr(), off.numel() - 1, _lib.ptr(ids), Q.data_ptr(), nq, probes.data_ptr(),
                                   nprobe, k, pos_base, D.data_ptr(), I.data_ptr(), cnt.data_ptr(), ws.data_ptr(),
                                   need if ws_bytes is None else ws_bytes, _lib.stream_ptr())
    return rc, D, I, cnt


def _scan_local(X, N, d, off, ids, Q, probes, k, pos_base):
    assert _lib.lib().wise_ivfl2_scan_local_workspace_bytes(probes.shape[0], probes.shape[1], k) > 0
    rc, D, I, cnt = _scan_local_raw(X, N, d, off, ids, Q, probes, k, pos_base)
    _lib.check(rc, "wise_ivfl2_scan_local")
    return D, I, cnt


class Slices:
    """The list-major arrays on the device, whole and cut into the clipped slices of every W of `worlds` (uploaded once)."""

    def __init__(self, X, ids, off, worlds=WORLDS):
        self.X, self.ids, self.off = X, ids, off
        self.N, self.d = X.shape
        self.whole = (_dev(X), _dev(off), _dev(ids))
        self.cut = {}
        for W in worlds:
            for r in range(W):
                lo, hi = shard_range(self.N, r, W)
                loff = np.clip(off - lo, 0, hi - lo)
                # a fresh allocation per slice: 16-byte aligned whatever lo is; a rank without rows holds no rows at all
                self.cut[W, r] = (lo, hi, loff, _dev(X[lo:hi]).reshape(hi - lo, self.d) if hi > lo else None, _dev(loff),
                                  _dev(ids[lo:hi]) if hi > lo else None)

    def emulate(self, Q, probes, k, worlds, with_ids):
        """Whole scan vs the merged NEGATED answers of W emulated ranks, probe_count against the host's count; -> the whole answer"""
        Qd, pd = _dev(Q), _dev(probes)
        xd, od, idd = self.whole
        Df, If = _scan_full(xd, od, idd if with_ids else None, Qd, pd, k)
        for W in worlds:
            Ds, Is = [], []
            for r in range(W):
                lo, hi, loff, x_d, o_d, i_d = self.cut[W, r]
                D, I, cnt = _scan_local(x_d, hi - lo, self.d, o_d, i_d if with_ids else None, Qd, pd, k, lo)
                want = np.where(probes >= 0, (loff[1:] > loff[:-1])[probes.clip(0)], False).sum(axis=1)
                assert np.array_equal(cnt.cpu().numpy(), want), (W, r)
                if hi == lo:
                    assert (I == -1).all() and (D == float(PAD)).all()
                Ds.append(-D)                                        # exact; the padding travels as the merge's own -3.4028235e38
                Is.append(I)
            Dm, Im = merge_device(torch.stack(Ds), torch.stack(Is), k)
            assert _same_bits(-Dm, Df) and _same_bits(Im, If), f"W={W} nq={probes.shape[0]} nprobe={probes.shape[1]} k={k} ids={with_ids}"
        return Df.cpu().numpy(), If.cpu().numpy()


@pytest.mark.parametrize("d", [16, 48, 512, 1024])
def test_emulated_ranks_give_the_bits_of_the_whole_scan(d):
    N, nlist = 3000, 37
    X, ids, off = _lists(N, d, nlist, seed=d)
    sizes = np.diff(off)
    assert (sizes == 0).any() and sizes.max() > 2 * sizes[sizes > 0].min()
    lists = np.repeat(np.arange(nlist), sizes)
    inside = [shard_range(N, r, W)[0] for W in WORLDS for r in range(1, W)]
    assert sum(lists[b] == lists[b - 1] for b in inside) >= 4          # slice boundaries that fall inside lists
    sl = Slices(X, ids, off)
    padded = False
    for n, (nq, nprobe, k) in enumerate((nq, nprobe, k) for nq in (1, 5) for nprobe in (1, 8, 64) for k in (1, 10, 100)):
        Q, probes = _queries(nq, d, nprobe, nlist, seed=1000 * d + n)
        assert (probes[:, nlist:] == -1).all()                          # nprobe = 64 > nlist: -1 padding
        for with_ids in (True, False):
            Df, If = sl.emulate(Q, probes, k, WORLDS, with_ids)
            padded |= bool((If == -1).any())
            if n % 6 == 4 and with_ids:                                 # (k = 10: one shape per nprobe against the restatement too)
                Dr, Ir = ref.scan(X, off, ids, Q, probes, k)
                assert np.array_equal(Df.view(np.int32), Dr.view(np.int32)) and np.array_equal(If, Ir)
    assert padded                                                       # a probed list shorter than k somewhere


def test_one_slice_equals_the_restatement():
    d, N, nlist, nq, nprobe, k = 48, 3000, 37, 3, 8, 100
    X, ids, off = _lists(N, d, nlist, seed=d + 1)
    Q, probes = _queries(nq, d, nprobe, nlist, seed=d + 2)
    lo, hi = shard_range(N, 1, 3)
    loff = np.clip(off - lo, 0, hi - lo)
    x_d = _dev(X[lo:hi]).reshape(hi - lo, d)
    D, I, _ = _scan_local(x_d, hi - lo, d, _dev(loff), _dev(ids[lo:hi]), _dev(Q), _dev(probes), k, lo)
    Dr, Ir = ref.scan(X[lo:hi], loff, ids[lo:hi], Q, probes, k)
    assert np.array_equal(D.cpu().numpy().view(np.int32), Dr.view(np.int32)) and np.array_equal(I.cpu().numpy(), Ir) and (Ir >= 0).any()
    D, I, _ = _scan_local(x_d, hi - lo, d, _dev(loff), None, _dev(Q), _dev(probes), k, lo)
    Dr, Ir = ref.scan(X[lo:hi], loff, None, Q, probes, k, pos_base=lo)
    assert np.array_equal(D.cpu().numpy().view(np.int32), Dr.view(np.int32))
    assert np.array_equal(I.cpu().numpy(), Ir) and (Ir[Ir >= 0] >= lo).all()      # positions in the whole array


def test_ties_across_a_boundary_keep_the_order_of_the_whole_scan():
    d, N = 48, 600
    off = np.array([0, 100, 350, 350, 520, 600], dtype=np.int64)
    rng = np.random.default_rng(8)
    X = ref.long_rows(N, d, 8)
    ids = rng.permutation(4 * N)[:N].astype(np.int64) + 5
    b2, b3 = shard_range(N, 1, 2)[0], shard_range(N, 1, 3)[0]          # 300 and 200: both inside list 1
    Q = ref.long_rows(2, d, 9)
    Q[1] = Q[0] * np.float32(1.01)
    tied = [b3 - 1, b3, b2 - 1, b2, 400, 401]                           # both sides of two boundaries in list 1, and list 3
    X[tied] = Q[0] * np.float32(1.005)                                  # one row six times, nearest to both queries by far
    probes = np.array([[3, 1, 0, -1], [1, 4, 3, 2]], dtype=np.int64)
    sl = Slices(X, ids, off, worlds=(2, 3, 8))
    for k in (4, 6, 10):
        for with_ids in (True, False):
            Df, If = sl.emulate(Q, probes, k, (2, 3, 8), with_ids)
            kk = min(k, 6)
            want = sorted(tied)[:kk]
            for q in range(2):
                assert (Df[q, :kk] == Df[q, 0]).all()
                assert list(If[q, :kk]) == (list(ids[want]) if with_ids else want)    # the row that comes first in X wins
            if k > 6:
                assert (Df[:, 6] > Df[:, 0]).all()


def test_ranks_without_rows_and_padding():
    d, nlist = 64, 6
    off = np.array([0, 2, 2, 2, 5, 5, 5], dtype=np.int64)              # two lists hold the 5 rows
    X = ref.long_rows(5, d, 9)
    ids = np.array([50, 40, 30, 20, 10], dtype=np.int64)
    Q, probes = _queries(3, d, 6, nlist, seed=4)                       # every list probed
    sl = Slices(X, ids, off)
    assert sum(1 for r in range(8) if sl.cut[8, r][3] is None) == 3    # W = 8 > 5 rows: three ranks hold nothing (X NULL)
    for with_ids in (True, False):
        Df, If = sl.emulate(Q, probes, 10, WORLDS, with_ids)
        assert (If[:, 5:] == -1).all() and (If[:, :5] >= 0).all()
        assert (Df[:, 5:].view(np.int32) == PAD.view(np.int32)).all()


# ------------------------------------------------------------------------------------------------------------------ capture, errors
def test_local_scan_under_graph_capture():
    d, N, nlist, nq, nprobe, k = 512, 3000, 37, 4, 8, 10
    X, ids, off = _lists(N, d, nlist, seed=3)
    Q, probes = _queries(nq, d, nprobe, nlist, seed=5)
    lo, hi = shard_range(N, 1, 3)
    args = (_dev(X[lo:hi]).reshape(hi - lo, d), hi - lo, d, _dev(np.clip(off - lo, 0, hi - lo)), _dev(ids[lo:hi]), _dev(Q), _dev(probes), k, lo)
    De, Ie, ce = _scan_local(*args)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D, I, c = _scan_local(*args)
    D.zero_()
    I.zero_()
    c.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert _same_bits(D, De) and _same_bits(I, Ie) and torch.equal(c, ce) and int((Ie >= 0).sum()) > 0


def test_unsupported_shapes_and_short_workspace_are_refused():
    lib = _lib.lib()
    d, N, nlist, nq, nprobe, k = 48, 300, 7, 2, 5, 10
    X, ids, off = _lists(N, d, nlist, seed=1)
    Q, probes = _queries(nq, d, nprobe, nlist, seed=2)
    x_d, o_d, i_d = _dev(X), _dev(off), _dev(ids)
    rest = (_dev(Q), _dev(probes))
    need = lib.wise_ivfl2_scan_local_workspace_bytes(nq, nprobe, k)
    for what, call in (
            (b"d=24", lambda: _scan_local_raw(x_d, N, 24, o_d, i_d, *rest, k, 0)),
            (b"k=2049", lambda: _scan_local_raw(x_d, N, d, o_d, i_d, *rest, 2049, 0)),
            (b"pos_base", lambda: _scan_local_raw(x_d, N, d, o_d, i_d, *rest, k, -1)),
            (b"workspace", lambda: _scan_local_raw(x_d, N, d, o_d, i_d, *rest, k, 0, ws_bytes=need - 1)),
            (b"null pointer", lambda: _scan_local_raw(None, N, d, o_d, i_d, *rest, k, 0)),
            (b"16-byte aligned", lambda: _scan_local_raw(x_d[1:].reshape(-1)[1:], N - 2, d, o_d, i_d, *rest, k, 0))):
        rc, D, I, cnt = call()
        assert rc == WISE_E_INVALID and what in lib.wise_last_error(), (what, rc, lib.wise_last_error())
        torch.cuda.synchronize()
        assert (D == 7.0).all() and (I == 7).all() and (cnt == -7).all()              # nothing ran: the outputs are untouched


# ------------------------------------------------------------------------------------------------------------------ index level
def test_index_slices_and_merge_equal_the_whole_index():
    from wise_amd.index.ivf_flat import IVFFlatL2Index
    from wise_amd.index.selector import IDSelectorRange
    from wise_amd.index.sharded import NO_SELECTOR, ShardedIVFFlatIPIndex

    d, N, nlist, k, W, nq = 64, 4096, 16, 20, 3, 5
    X = ref.long_rows(N, d, 21, centres=16)
    ids = np.random.default_rng(1).permutation(3 * N)[:N].astype(np.int64)
    full = IVFFlatL2Index(d, nlist)
    full.niter = 3
    full.train(X)
    full.add_with_ids(X, ids)
    full.nprobe = 6
    c, Xs, ids_s, off = full.lists_host()
    Q = _dev(X[:nq] + np.float32(0.05) * np.random.default_rng(2).standard_normal((nq, d)).astype(np.float32))
    Dw, Iw = full.search_device(Q, k)
    locs = []
    for r in range(W):
        lo, hi = shard_range(N, r, W)
        loc = IVFFlatL2Index(d, nlist)
        loc.set_centroids(c)
        loc.adopt_lists(torch.from_numpy(Xs[lo:hi]), torch.from_numpy(ids_s[lo:hi]), torch.from_numpy(np.clip(off - lo, 0, hi - lo)),
                        pos_base=lo)
        loc.nprobe = 6
        assert loc.pos_base == lo and loc.ntotal == hi - lo and loc.is_trained
        locs.append(loc)
    cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
    parts = [loc.search_local_device(Q, k, probe_count=cnt) for loc in locs]
    assert 0 < int(cnt.max()) <= 6
    Dm, Im = merge_device(torch.stack([-p[0] for p in parts]), torch.stack([p[1] for p in parts]), k)
    assert _same_bits(-Dm, Dw) and _same_bits(Im, Iw) and int((Iw >= 0).sum()) == nq * k
    pos = [loc.search_local_device(Q, k, positions=True) for loc in locs]
    Dp, Ip = merge_device(torch.stack([-p[0] for p in pos]), torch.stack([p[1] for p in pos]), k)
    assert _same_bits(-Dp, Dw) and torch.equal(_dev(ids_s)[Ip], Iw)     # positions=True: the positions of the whole array
    want = np.array([ids_s[0], ids_s[N - 1], 3 * N + 9, ids_s[shard_range(N, 1, W)[0]], ids_s[2000]], dtype=np.int64)
    whole = full.reconstruct_batch(want)
    mine = np.stack([loc.reconstruct_batch(want) for loc in locs])       # [W, n, d]
    have = ~np.isnan(mine[:, :, 0])
    assert list(have.sum(axis=0)) == [1, 1, 0, 1, 1]
    merged = mine[have.argmax(axis=0), np.arange(len(want))]
    assert np.array_equal(merged.view(np.int32), whole.view(np.int32)) and np.isnan(whole[2]).all() and np.isfinite(whole[0]).all()
    # the wrapper outside a process group: the local answer, distances as they are
    w = ShardedIVFFlatIPIndex(locs[1])
    assert w.nlist == nlist and w.is_trained and w.nprobe == 6 and w.ntotal == locs[1].ntotal and w.local.metric == "l2"
    D1, I1 = w.search_device(Q, k)
    assert _same_bits(D1, parts[1][0]) and _same_bits(I1, parts[1][1])
    with pytest.raises(NotImplementedError) as e:
        w.search_device(Q, k, sel=IDSelectorRange(0, 10))
    assert str(e.value) == NO_SELECTOR
    with pytest.raises(NotImplementedError):
        w.range_search(Q.cpu().numpy(), 0.5)
    with pytest.raises(NotImplementedError):
        w.remove_ids(ids[:3])
    with pytest.raises(NotImplementedError, match="pos_base"):
        locs[1].remove_ids(ids[:3])
    with pytest.raises(NotImplementedError):
        locs[1]._scan(Q, k, True, None, sel=IDSelectorRange(0, 10))       # a rank's share of a search takes no selector


# ------------------------------------------------------------------------------------------------------------------ RCCL
def test_sharded_plugin_over_rccl_world1(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "sharded_ivf_l2_nccl_worker.py"), str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert res["ok"], json.dumps(res)
    nq, k = 3, 10
    assert res["exchange_bytes"] == 16 * nq * k                                      # one exchange of (score, id) planes

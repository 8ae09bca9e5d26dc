"""-m gpu: IndexIVFOPQ<m> and its R8 / R16 forms sharded across ranks.  The sharded classes are ShardedIVFPQIPIndex /
ShardedIVFPQRefineIPIndex (wise_amd/index/sharded.py) around IVFOPQIPIndex / IVFOPQRefineIPIndex: the rotation is replicated and
each rank rotates the query itself, so the kernels a rank runs on its slice are those tests/test_gpu_ivfpq_sharded.py already
holds to the whole-index scan.  Here:
(1) one process, emulated ranks: local OPQ indexes over W clipped slices + wise_topk_merge give the bits of the whole OPQ index;
(2) the plugin path on RCCL at world size 1 with the short-cut off, in a child process with its own time limit
    (tests/sharded_ivfopq_nccl_worker.py)."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import ivfopq_ref
from wise_amd.index.ivf_pq import IVFOPQIPIndex, IVFOPQRefineIPIndex
from wise_amd.index.sharded import merge_device, shard_range

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32) if a.dtype == torch.float32 else a,
                                              b.contiguous().view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.parametrize("kind", [None, 8, 16])
def test_index_slices_and_merge_equal_the_whole_index(kind):
    d, m, N, nlist, k, W, nq = 64, 16, 20000, 128, 20, 4, 5
    X = ivfopq_ref.decaying_spectrum_rows(N, d, 64, 0.5, seed=11)
    ids = np.random.default_rng(1).permutation(3 * N)[:N].astype(np.int64)
    full = IVFOPQIPIndex(d, nlist, m) if kind is None else IVFOPQRefineIPIndex(d, nlist, m, kind, 20)
    full.opq_niter = 5
    full.train(X[:8000])
    full.add_with_ids(X, ids)
    full.nprobe = 24
    c, cb, codes, ids_s, off = full.lists_host()
    Qh = X[:nq] + 0.05 * np.random.default_rng(2).standard_normal((nq, d)).astype(np.float32)
    Q = _dev((Qh / np.linalg.norm(Qh, axis=1, keepdims=True)).astype(np.float32))
    Dw, Iw = full.search_device(Q, k)
    locs = []
    for r in range(W):
        lo, hi = shard_range(N, r, W)
        loff = torch.from_numpy(np.clip(off - lo, 0, hi - lo))
        if kind is None:
            loc = IVFOPQIPIndex(d, nlist, m)
            loc.adopt_lists(torch.from_numpy(codes[lo:hi]), torch.from_numpy(ids_s[lo:hi]), loff, pos_base=lo)
        else:
            rows, scales = full.store_host()
            loc = IVFOPQRefineIPIndex(d, nlist, m, kind, k_factor=20)
            loc.adopt_lists(torch.from_numpy(codes[lo:hi]), torch.from_numpy(ids_s[lo:hi]), loff,
                            torch.from_numpy(rows[lo:hi] if kind == 8 else rows[lo:hi].view(np.int16)),
                            None if scales is None else torch.from_numpy(scales[lo:hi]), pos_base=lo)
        loc.set_centroids(c)
        loc.set_codebooks(cb)
        assert not loc.is_trained                             # no rotation yet
        loc.set_rotation(full.rotation.cpu().numpy())
        loc.nprobe = 24
        locs.append(loc)
    if kind is None:
        parts = [loc.search_local_device(Q, k) for loc in locs]
    else:
        kc = full.candidates(k)
        cands = [loc.candidates_local_device(Q, kc) for loc in locs]
        _, gc = merge_device(torch.stack([p[0] for p in cands]), torch.stack([p[1] for p in cands]), kc)
        parts = [loc.refine_local_device(Q, gc, k) for loc in locs]
    Dm, Im = merge_device(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]), k)
    assert _same_bits(Dm, Dw) and _same_bits(Im, Iw) and int((Iw >= 0).sum()) == nq * k


def test_sharded_ivfopq_plugin_over_rccl_world1(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "sharded_ivfopq_nccl_worker.py"), str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + "\n" + p.stderr[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert res["ok"], json.dumps(res)
    nq, k = 3, 10
    assert res["exchange_bytes"]["IndexIVFOPQ16"] == 16 * nq * k                     # one exchange: the rotation adds none
    for t in ("IndexIVFOPQ16R8", "IndexIVFOPQ16R16"):
        assert res["exchange_bytes"][t] == 16 * nq * (res["candidates"] + k)         # candidates, then re-ranked answers
    assert res["candidates"] == 500

"""CPU tests (-m "not gpu") of the IndexIVFFlat sharded across ranks (wise_amd/index/sharded.py ShardedIVFFlatIPIndex):
the ranged reader of the list-major file, and the multi-rank build / load / collective search through the plugin surface
(SearchIndexFactory) at world size 2 over gloo.  The rows of a rank live in a numpy stand-in for IVFFlatIPIndex here
(its local scan and the merge are the stand-in's); tests/test_gpu_ivf_sharded.py runs the HIP kernels and RCCL."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parent.parent
NEG = np.float32(-3.4028234663852886e38)
FID = "mlfoundations/open_clip/ViT-B-32/seeded-0"


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ---------------------------------------------------------------------------------------------------------------------
# faiss_io.read_ivf_flat_ip_range
def _ivf_file(path, sizes, d, seed):
    from wise_amd.index import faiss_io

    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    n = int(sizes.sum())
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    X = rng.standard_normal((n, d)).astype(np.float32)
    ids = rng.permutation(10 * n + 1)[:n].astype(np.int64) + 3
    c = rng.standard_normal((len(sizes), d)).astype(np.float32)
    faiss_io.write_ivf_flat_ip(path, c, X, ids, off, nprobe=7)
    return c, X, ids, off


@pytest.mark.parametrize("sizes", [
    [5, 0, 0, 17, 1, 0, 9, 0, 0, 0, 3, 12],           # most lists empty ('sprs' layout), lists straddle boundaries
    [40, 3, 8, 2, 11, 6, 1, 4, 9, 2],                 # 'full' layout, one list larger than a rank's share
    [0, 0, 0, 6, 0, 0],                               # one non-empty list: all ranks cut the same list
    [0, 0, 0],                                        # no rows at all
])
def test_read_ivf_flat_ip_range_tiles_the_file(tmp_path, sizes):
    from wise_amd.index import faiss_io
    from wise_amd.index.sharded import shard_range

    fn = tmp_path / "x.faiss"
    c, X, ids, off = _ivf_file(fn, sizes, 8, seed=len(sizes))
    full = faiss_io.read_ivf_flat_ip(fn)
    assert np.array_equal(full["X"], X) and np.array_equal(full["list_off"], off)
    n = X.shape[0]
    assert faiss_io.ivf_flat_ip_ntotal(fn) == n
    for W in (1, 2, 3, 8):
        parts = []
        for r in range(W):
            lo, hi = shard_range(n, r, W)
            p = faiss_io.read_ivf_flat_ip_range(fn, lo, hi)
            assert np.array_equal(p["centroids"], c) and p["nprobe"] == 7
            assert p["X"].shape == (hi - lo, 8) and p["ids"].shape == (hi - lo,)
            assert np.array_equal(p["list_off"], np.clip(off - lo, 0, hi - lo)), (W, r)
            parts.append(p)
        assert np.array_equal(np.concatenate([p["X"] for p in parts]), full["X"]), W
        assert np.array_equal(np.concatenate([p["ids"] for p in parts]), full["ids"]), W
        assert np.array_equal(sum(p["list_off"] for p in parts), full["list_off"]), W    # the clipped offsets add up


def test_read_ivf_flat_ip_range_reads_only_the_overlapping_lists(tmp_path, monkeypatch):
    from wise_amd.index import faiss_io

    fn = tmp_path / "x.faiss"
    sizes = [50, 50, 50, 50]
    c, X, ids, off = _ivf_file(fn, sizes, 16, seed=1)
    counts = []
    real = np.fromfile
    monkeypatch.setattr(faiss_io.np, "fromfile", lambda *a, **k: counts.append(k.get("count", -1)) or real(*a, **k))
    p = faiss_io.read_ivf_flat_ip_range(fn, 60, 90)                   # inside list 1
    assert np.array_equal(p["X"], X[60:90]) and np.array_equal(p["ids"], ids[60:90])
    assert sum(counts) - 4 * 16 - 4 == 30 * 16 + 30                    # centroids + list sizes, then 30 rows and 30 ids
    with pytest.raises(ValueError):
        faiss_io.read_ivf_flat_ip_range(fn, 10, 201)


# ---------------------------------------------------------------------------------------------------------------------
# the plugin surface at world size 2 (gloo) with a numpy stand-in for IVFFlatIPIndex
class _DirectMap:
    def __init__(self):
        self.type = 0


def _scores(X, q):
    return (X.astype(np.float64) @ q.astype(np.float64)).astype(np.float32)     # per row: independent of the slice


class _CpuIVF:
    """What FeatureSearchIndex.ivf_index_factory must offer: train / centroids / set_centroids / assign / adopt_lists /
    nprobe / search_local_device / reconstruct_batch (and merge_lists for the wrapper's merge)."""

    def __init__(self, d, nlist):
        self.d, self.nlist, self.device = int(d), int(nlist), torch.device("cpu")
        self.nprobe, self.parallel_mode, self.direct_map, self.is_trained = 1, 0, _DirectMap(), False
        self.centroids = None
        self.X, self.ids, self.list_off = np.zeros((0, d), np.float32), np.zeros(0, np.int64), np.zeros(nlist + 1, np.int64)

    def train(self, x):
        c = np.asarray(x, np.float64)[:self.nlist]                   # deterministic stand-in for k-means
        self.set_centroids((c / np.linalg.norm(c, axis=1, keepdims=True)).astype(np.float32))

    def set_centroids(self, c):
        self.centroids = np.array(c, dtype=np.float32)
        self.is_trained = True

    def assign(self, x):
        return (np.asarray(x, np.float64) @ self.centroids.astype(np.float64).T).argmax(axis=1).astype(np.int64)

    def adopt_lists(self, X, ids, list_off):
        self.X, self.ids, self.list_off = X.numpy().copy(), ids.numpy().copy(), list_off.numpy().copy()
        return self

    @property
    def ntotal(self):
        return self.X.shape[0]

    def make_direct_map(self, enable=True):
        self.direct_map.type = 2 if enable else 0

    def search_local_device(self, q, k):
        from oracle import ivf_ref

        Q = q.numpy()
        probes = ivf_ref.coarse_probes(self.centroids, Q, min(self.nprobe, self.nlist))
        D = np.full((Q.shape[0], k), NEG, np.float32)
        I = np.full((Q.shape[0], k), -1, np.int64)
        for i in range(Q.shape[0]):
            rows = np.concatenate([np.arange(self.list_off[l], self.list_off[l + 1]) for l in probes[i]] +
                                  [np.zeros(0, np.int64)]).astype(np.int64)
            s = _scores(self.X[rows], Q[i])
            o = np.lexsort((rows, -s.astype(np.float64)))[:k]
            D[i, :len(o)], I[i, :len(o)] = s[o], self.ids[rows[o]]
        return torch.from_numpy(D), torch.from_numpy(I)

    def reconstruct_batch(self, want):
        out = np.full((len(want), self.d), np.nan, np.float32)
        for i, w in enumerate(want):
            hit = np.flatnonzero(self.ids == w)
            if len(hit):
                out[i] = self.X[hit[0]]
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


QUERIES = ["dog", "cat", "a red car", "bird"]


def _collect(si, d, N):
    Q = np.random.default_rng(6).standard_normal((3, d)).astype(np.float32)
    out = {}
    out["dist"], out["ids"] = si.search("video", "dog", topk=7)
    sb = si.search_batch("video", QUERIES, topk=9)
    out["sb_D"], out["sb_I"] = np.stack([a for a, _ in sb]), np.stack([b for _, b in sb])
    out["D"], out["I"] = si.index.search(Q, 25)
    out["rec"] = si.index.reconstruct_batch(np.array([1, N, 500, N + 5], dtype=np.int64))
    out["ntotal"] = np.array([si.index.ntotal])
    return out


def _plugin_worker(rank, world, port, root, N, d):
    sys.path.insert(0, str(ROOT))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["WISE_SHARDED_IVF"] = "1"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import wise_amd.index.feature_search_index as fsi
    from wise_amd.index import faiss_io
    from wise_amd.index.search_index_factory import SearchIndexFactory
    from wise_amd.index.sharded import ShardedIVFFlatIPIndex

    fsi.FeatureSearchIndex.ivf_index_factory = _CpuIVF
    fsi.FeatureExtractorFactory = lambda fid: _FakeTextTower(d)
    root = Path(root)
    out = {}
    # (A) the collective build: own store shards -> one part file per rank -> load the part
    si = SearchIndexFactory("video", FID, {"features_dir": root / "features", "index_dir": root / "index_parts"})
    si.create_index("IndexIVFFlat")
    part = si.get_index_part_filename("IndexIVFFlat", rank, world)
    assert part.exists() and not si.get_index_filename("IndexIVFFlat").exists()
    dist.barrier()
    assert si.load_index("IndexIVFFlat") is True
    assert isinstance(si.index, ShardedIVFFlatIPIndex)
    idx = si.index
    assert idx.is_trained and idx.d == d and idx.parallel_mode == 0
    idx.parallel_mode = 1                                                # api/routes.py:899-909
    idx.nprobe = 8
    idx.make_direct_map(True)
    assert idx.local.nprobe == 8 and idx.nprobe == 8 and idx.local.parallel_mode == 1 and idx.direct_map.type == 2
    out.update({"A_" + k: v for k, v in _collect(si, d, N).items()})
    # (B) rank 0 lays the parts end to end into one file; every rank then loads its range of that file
    if rank == 0:
        ps = [faiss_io.read_ivf_flat_ip(si.get_index_part_filename("IndexIVFFlat", r, world)) for r in range(world)]
        (root / "index_single").mkdir()
        faiss_io.write_ivf_flat_ip(root / "index_single" / "video-IndexIVFFlat.faiss", ps[0]["centroids"],
                                   np.concatenate([p["X"] for p in ps]), np.concatenate([p["ids"] for p in ps]),
                                   sum(p["list_off"] for p in ps), nprobe=8)
    dist.barrier()
    si2 = SearchIndexFactory("video", FID, {"features_dir": root / "features", "index_dir": root / "index_single"})
    assert si2.load_index("IndexIVFFlat") is True
    assert isinstance(si2.index, ShardedIVFFlatIPIndex) and si2.index.nprobe == 8
    out.update({"B_" + k: v for k, v in _collect(si2, d, N).items()})
    out["B_list_off"] = si2.index.local.list_off
    np.savez(root / f"ivf_rank{rank}.npz", **out)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_ivf_through_the_plugin_surface_world2(tmp_path):
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    from wise_amd.index import faiss_io
    from wise_amd.index.ivf_flat import reference_nlist
    from wise_amd.index.sharded import shard_range

    N, d, world = 1001, 32, 2
    X = np.random.default_rng(5).standard_normal((N, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X[700] = X[20]                                                       # equal scores on both ranks' rows
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
    assert len(idcat) == N
    nlist = reference_nlist(N)
    ref = _CpuIVF(d, nlist)
    sample = np.sort(np.random.default_rng(1234).permutation(N)[:min(N, 100 * nlist)])
    ref.train(Xcat[sample])
    a = ref.assign(Xcat)
    order = np.argsort(a, kind="stable")
    Xl, idl = Xcat[order], idcat[order]
    off = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=nlist))]).astype(np.int64)
    parts = []
    for r in range(world):
        p = faiss_io.read_ivf_flat_ip(tmp_path / "index_parts" / f"video-IndexIVFFlat.faiss.part-{r:03d}-of-{world:03d}")
        lo, hi = shard_range(N, r, world)
        assert p["centroids"].tobytes() == ref.centroids.tobytes(), r          # the same centroid bits on every rank
        assert np.array_equal(p["X"], Xl[lo:hi]) and np.array_equal(p["ids"], idl[lo:hi]), r
        assert np.array_equal(p["list_off"], np.clip(off - lo, 0, hi - lo)), r
        parts.append(p)
    # one single-process stand-in over all rows answers what the collective search answers
    ref.adopt_lists(torch.from_numpy(Xl), torch.from_numpy(idl), torch.from_numpy(off))
    ref.nprobe = 8
    tower = _FakeTextTower(d)
    q1 = tower.extract_text_features(["This is a photo of a dog"])
    D1, I1 = (t.numpy() for t in ref.search_local_device(torch.from_numpy(q1), 7))
    qb = tower.extract_text_features(["This is a photo of a " + s for s in QUERIES])
    Db, Ib = (t.numpy() for t in ref.search_local_device(torch.from_numpy(qb), 9))
    Q = np.random.default_rng(6).standard_normal((3, d)).astype(np.float32)
    D3, I3 = (t.numpy() for t in ref.search_local_device(torch.from_numpy(Q), 25))
    assert (I3 >= 0).all() and (I1 >= 0).all()
    for r in range(world):
        g = np.load(tmp_path / f"ivf_rank{r}.npz")
        for tag in "AB":
            assert np.array_equal(g[f"{tag}_ids"], I1[0]) and np.array_equal(g[f"{tag}_dist"], D1[0]), (r, tag)
            assert np.array_equal(g[f"{tag}_sb_I"], Ib) and np.array_equal(g[f"{tag}_sb_D"], Db), (r, tag)
            assert np.array_equal(g[f"{tag}_I"], I3) and np.array_equal(g[f"{tag}_D"], D3), (r, tag)
            rec = g[f"{tag}_rec"]
            assert np.array_equal(rec[0], X[0]) and np.array_equal(rec[1], X[N - 1]) and np.array_equal(rec[2], X[499])
            assert np.isnan(rec[3]).all()
            assert int(g[f"{tag}_ntotal"][0]) == N
        lo, hi = shard_range(N, r, world)
        assert np.array_equal(g["B_list_off"], np.clip(off - lo, 0, hi - lo))

"""CPU tests (-m "not gpu") of IndexIVFPQ<m> / IndexIVFPQ<m>R8 / R16 sharded across ranks (wise_amd/index/sharded.py
ShardedIVFPQIPIndex, ShardedIVFPQRefineIPIndex): the ranged readers of the 'IwPQ' and 'WiPR' files, and the multi-rank build /
load / collective search through the plugin surface (SearchIndexFactory) at world size 2 over gloo.  A rank's rows live in numpy
stand-ins built on tests/ivfpq_ref.py and tests/ivfpq_refine_ref.py here; tests/test_gpu_ivfpq_sharded.py runs the HIP kernels
and RCCL."""
import os
import shutil
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ivfpq_ref
import ivfpq_refine_ref as rr

ROOT = Path(__file__).resolve().parent.parent
NEG = np.float32(-3.4028234663852886e38)
FID = "mlfoundations/open_clip/ViT-B-32/seeded-0"
TYPES = ("IndexIVFPQ8", "IndexIVFPQ8R8", "IndexIVFPQ8R16")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ---------------------------------------------------------------------------------------------------------------------
# faiss_io.read_ivf_pq_ip_range / read_ivf_pq_refine_ip_range
def _pq_file(path, sizes, d, m, seed, kind=None):
    from wise_amd.index import faiss_io

    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    n = int(sizes.sum())
    f = {"list_off": np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
         "codes": rng.integers(0, 256, size=(n, m), dtype=np.uint8),
         "ids": rng.permutation(10 * n + 1)[:n].astype(np.int64) + 3,
         "centroids": rng.standard_normal((len(sizes), d)).astype(np.float32),
         "codebooks": rng.standard_normal((m, 256, d // m)).astype(np.float32)}
    head = (f["centroids"], f["codebooks"], f["codes"], f["ids"], f["list_off"])
    if kind is None:
        faiss_io.write_ivf_pq_ip(path, *head, nprobe=7)
    else:
        f["rows"], f["scales"] = rr.quantise(rng.standard_normal((n, d)).astype(np.float32), kind)
        faiss_io.write_ivf_pq_refine_ip(path, *head, kind, 20, f["rows"], f["scales"], nprobe=7)
    return f


def _readers(kind):
    from wise_amd.index import faiss_io

    if kind is None:
        return faiss_io.read_ivf_pq_ip, faiss_io.read_ivf_pq_ip_range, faiss_io.ivf_pq_ip_ntotal
    return faiss_io.read_ivf_pq_refine_ip, faiss_io.read_ivf_pq_refine_ip_range, faiss_io.ivf_pq_refine_ip_ntotal


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
    w = _pq_file(fn, sizes, d, m, seed=len(sizes), kind=kind)
    read, read_range, ntotal = _readers(kind)
    full = read(fn)
    n = w["codes"].shape[0]
    assert np.array_equal(full["codes"], w["codes"]) and np.array_equal(full["list_off"], w["list_off"]) and ntotal(fn) == n
    arrays = ["codes", "ids"] + ([] if kind is None else ["rows"]) + (["scales"] if kind == 8 else [])
    for W in (1, 2, 3, 8):
        parts = []
        for r in range(W):
            lo, hi = shard_range(n, r, W)
            p = read_range(fn, lo, hi)
            assert np.array_equal(p["centroids"], w["centroids"]) and np.array_equal(p["codebooks"], w["codebooks"]) and p["nprobe"] == 7
            assert p["codes"].shape == (hi - lo, m) and p["ids"].shape == (hi - lo,)
            assert np.array_equal(p["list_off"], np.clip(w["list_off"] - lo, 0, hi - lo)), (W, r)
            if kind is not None:
                assert p["kind"] == kind and p["k_factor"] == 20 and p["rows"].shape == (hi - lo, d) and p["rows"].dtype == w["rows"].dtype
                assert (p["scales"] is None) == (kind == 16)
            parts.append(p)
        for a in arrays:
            assert np.array_equal(np.concatenate([p[a] for p in parts]), w[a]), (W, a)
        assert np.array_equal(sum(p["list_off"] for p in parts), full["list_off"]), W    # the clipped offsets add up


@pytest.mark.parametrize("kind", [None, 8, 16])
def test_range_readers_read_only_the_overlapping_lists(tmp_path, monkeypatch, kind):
    from wise_amd.index import faiss_io

    fn = tmp_path / "x.faiss"
    d, m = 16, 4
    w = _pq_file(fn, [50, 50, 50, 50], d, m, seed=1, kind=kind)
    _, read_range, _ = _readers(kind)
    counts = []
    real = np.fromfile
    monkeypatch.setattr(faiss_io.np, "fromfile", lambda *a, **k: counts.append(k.get("count", -1)) or real(*a, **k))
    p = read_range(fn, 60, 90)                                        # inside list 1
    assert np.array_equal(p["codes"], w["codes"][60:90]) and np.array_equal(p["ids"], w["ids"][60:90])
    payload = 30 * m + 30                                             # 30 rows of codes and 30 ids
    if kind is not None:
        assert np.array_equal(p["rows"], w["rows"][60:90])
        payload += 30 * d + (30 if kind == 8 else 0)                  # 30 compact rows (and 30 scales)
        if kind == 8:
            assert np.array_equal(p["scales"], w["scales"][60:90])
    assert sum(counts) - 4 * d - 256 * d - 4 == payload               # centroids + codebooks + list sizes, then the slice
    with pytest.raises(ValueError):
        read_range(fn, 10, 201)


# ---------------------------------------------------------------------------------------------------------------------
# the plugin surface at world size 2 (gloo) with numpy stand-ins for IVFPQIPIndex / IVFPQRefineIPIndex
class _DirectMap:
    def __init__(self):
        self.type = 0


class _CpuIVFPQ:
    """What FeatureSearchIndex.ivfpq_index_factory must offer: train / centroids / codebooks / set_centroids / set_codebooks /
    encode_rows / adopt_lists(pos_base) / nprobe / search_local_device / reconstruct_batch (and merge_lists for the wrapper)."""
    kind = None

    def __init__(self, d, nlist, m):
        self.d, self.nlist, self.m, self.device = int(d), int(nlist), int(m), torch.device("cpu")
        self.nprobe, self.parallel_mode, self.direct_map = 1, 0, _DirectMap()
        self.centroids = self.codebooks = None
        self.codes, self.ids, self.list_off, self.pos_base = np.zeros((0, m), np.uint8), np.zeros(0, np.int64), np.zeros(nlist + 1, np.int64), 0

    @property
    def is_trained(self):
        return self.centroids is not None and self.codebooks is not None

    def train(self, x):
        x = np.asarray(x, np.float64)
        c = x[:self.nlist]                                            # deterministic stand-in for k-means
        self.set_centroids((c / np.linalg.norm(c, axis=1, keepdims=True)).astype(np.float32))
        x = x[:512].astype(np.float32)
        self.set_codebooks(ivfpq_ref.train(x - self.centroids[self._assign(x)], self.m, niter=2).astype(np.float32))

    def set_centroids(self, c):
        self.centroids = np.array(c, dtype=np.float32)

    def set_codebooks(self, cb):
        self.codebooks = np.array(cb, dtype=np.float32)

    def _assign(self, x):
        return (np.asarray(x, np.float64) @ self.centroids.astype(np.float64).T).argmax(axis=1).astype(np.int64)

    def _extra(self, x):
        return ()

    def encode_rows(self, x):
        x = np.asarray(x, np.float32)
        a = self._assign(x)
        return (a, ivfpq_ref.encode(x - self.centroids[a], self.codebooks), *self._extra(x))

    def adopt_lists(self, codes, ids, list_off, pos_base=0):
        self.codes, self.ids, self.list_off, self.pos_base = codes.numpy().copy(), ids.numpy().copy(), list_off.numpy().copy(), int(pos_base)
        return self

    @property
    def ntotal(self):
        return self.codes.shape[0]

    def hbm_bytes(self):
        return self.codes.nbytes + self.ids.nbytes

    def make_direct_map(self, enable=True):
        self.direct_map.type = 2 if enable else 0

    def _scan(self, Q, k, positions):
        from oracle import ivf_ref

        probes = ivf_ref.coarse_probes(self.centroids, Q, min(self.nprobe, self.nlist))
        coarse = Q.astype(np.float64) @ self.centroids.astype(np.float64).T        # per (query, list): independent of the slice
        bias = np.take_along_axis(coarse, probes, axis=1).astype(np.float32)
        D, I = ivfpq_ref.scan(self.codes, self.list_off, None if positions else self.ids, ivfpq_ref.lut(Q, self.codebooks).astype(np.float32),
                              probes, bias, k)
        return D, (np.where(I >= 0, I + self.pos_base, -1) if positions else I)

    def search_local_device(self, q, k, probe_count=None, positions=False):
        D, I = self._scan(q.numpy(), k, positions)
        return torch.from_numpy(D), torch.from_numpy(I)

    search_device = search_local_device

    def reconstruct_batch(self, want):
        out = np.full((len(want), self.d), np.nan, np.float32)
        lists = ivfpq_ref.list_of_rows(self.list_off)
        for i, w in enumerate(want):
            hit = np.flatnonzero(self.ids == w)
            if len(hit):
                out[i] = self._row(hit[:1], lists)
        return out

    def _row(self, pos, lists):
        return ivfpq_ref.decode(self.codes[pos], lists[pos], self.centroids, self.codebooks)

    @staticmethod
    def merge_lists(Ds, Is, k):
        from oracle import ip_topk_ref
        D, I = ip_topk_ref.merge_topk(Ds.numpy(), Is.numpy(), k)
        return torch.from_numpy(D), torch.from_numpy(I)


class _CpuIVFPQRefine(_CpuIVFPQ):
    """... and ivfpq_refine_index_factory: the two phases, candidates_local_device and refine_local_device."""

    def __init__(self, d, nlist, m, kind, k_factor=50):
        super().__init__(d, nlist, m)
        self.kind, self.k_factor = int(kind), int(k_factor)
        self.rows, self.scales = None, None

    def _extra(self, x):
        rows, scales = rr.quantise(x, self.kind)
        return (rows, scales) if self.kind == 8 else (rows.view(np.int16),)

    def adopt_lists(self, codes, ids, list_off, rows=None, scales=None, pos_base=0):
        super().adopt_lists(codes, ids, list_off, pos_base)
        self.rows = rows.numpy().copy() if self.kind == 8 else rows.numpy().view(np.uint16).copy()
        self.scales = None if scales is None else scales.numpy().copy()
        return self

    def hbm_bytes(self):
        return super().hbm_bytes() + self.rows.nbytes

    def candidates(self, k):
        return max(k, min(k * max(self.k_factor, 1), 2048))

    def candidates_local_device(self, q, kc):
        D, I = self._scan(q.numpy(), kc, True)
        return torch.from_numpy(D), torch.from_numpy(I)

    def refine_local_device(self, q, cand, k):
        local = np.where(cand.numpy() >= 0, cand.numpy() - self.pos_base, -1)         # outside the slice: a hole
        D, I = rr.refine(self.rows, self.kind, self.scales, self.ids, q.numpy(), local, k)
        return torch.from_numpy(D), torch.from_numpy(I)

    def search_device(self, q, k):
        return self.refine_local_device(q, self.candidates_local_device(q, self.candidates(k))[1], k)

    def search_local_device(self, q, k, probe_count=None, positions=False):
        raise NotImplementedError

    def _row(self, pos, lists):
        return rr.dequantise(self.rows[pos], self.kind, None if self.scales is None else self.scales[pos])


class _FakeTextTower:
    def __init__(self, d):
        self.d = d

    def extract_text_features(self, texts):
        import zlib
        out = np.stack([np.random.default_rng(zlib.crc32(t.encode())).standard_normal(self.d) for t in texts])
        return (out / np.linalg.norm(out, axis=1, keepdims=True)).astype(np.float32)


QUERIES = ["dog", "cat", "a red car", "bird"]
WANT_IDS = [1, 1001, 500, 1006]


def _collect(si, d):
    Q = np.random.default_rng(6).standard_normal((3, d)).astype(np.float32)
    out = {}
    out["dist"], out["ids"] = si.search("video", "dog", topk=7)
    sb = si.search_batch("video", QUERIES, topk=9)
    out["sb_D"], out["sb_I"] = np.stack([a for a, _ in sb]), np.stack([b for _, b in sb])
    out["D"], out["I"] = si.index.search(Q, 25)
    out["rec"] = si.index.reconstruct_batch(np.array(WANT_IDS, dtype=np.int64))
    out["ntotal"] = np.array([si.index.ntotal])
    out["xbytes"] = np.array([si.index.last_exchange_bytes])
    return out


def _plugin_worker(rank, world, port, root, N, d):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["WISE_SHARDED_IVF"] = "1"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import wise_amd.index.feature_search_index as fsi
    from wise_amd.index import faiss_io
    from wise_amd.index.search_index_factory import SearchIndexFactory
    from wise_amd.index.sharded import ShardedIVFPQIPIndex, ShardedIVFPQRefineIPIndex, shard_range

    fsi.FeatureSearchIndex.ivfpq_index_factory = _CpuIVFPQ
    fsi.FeatureSearchIndex.ivfpq_refine_index_factory = _CpuIVFPQRefine
    fsi.FeatureExtractorFactory = lambda fid: _FakeTextTower(d)
    root = Path(root)
    out = {}
    for itype in TYPES:
        refine = itype != TYPES[0]
        read = faiss_io.read_ivf_pq_refine_ip if refine else faiss_io.read_ivf_pq_ip
        # (A) the collective build: own store shards -> one part file per rank -> load the part
        si = SearchIndexFactory("video", FID, {"features_dir": root / "features", "index_dir": root / "index_parts"})
        si.create_index(itype)
        part = si.get_index_part_filename(itype, rank, world)
        assert part.exists() and not si.get_index_filename(itype).exists()
        dist.barrier()
        assert si.load_index(itype) is True
        idx = si.index
        assert type(idx) is (ShardedIVFPQRefineIPIndex if refine else ShardedIVFPQIPIndex)
        assert idx.is_trained and idx.d == d and idx.local.pos_base == shard_range(N, rank, world)[0]
        idx.nprobe = 8
        idx.make_direct_map(True)
        assert idx.local.nprobe == 8 and idx.direct_map.type == 2 and idx.hbm_bytes() == idx.local.hbm_bytes()
        if refine:
            idx.k_factor = 6
            assert idx.local.k_factor == 6
        out.update({f"{itype}_A_{k}": v for k, v in _collect(si, d).items()})
        # (B) rank 0 lays the parts end to end into one file; every rank then loads its range of that file
        sdir = root / ("index_single_" + itype)
        if rank == 0:
            ps = [read(si.get_index_part_filename(itype, r, world)) for r in range(world)]
            sdir.mkdir()
            cat = lambda a: np.concatenate([p[a] for p in ps])
            head = (ps[0]["centroids"], ps[0]["codebooks"], cat("codes"), cat("ids"), sum(p["list_off"] for p in ps))
            fn = sdir / si.get_index_filename(itype).name
            if refine:
                faiss_io.write_ivf_pq_refine_ip(fn, *head, ps[0]["kind"], 6, cat("rows"), None if ps[0]["scales"] is None else cat("scales"),
                                                nprobe=8)
            else:
                faiss_io.write_ivf_pq_ip(fn, *head, nprobe=8)
        dist.barrier()
        si2 = SearchIndexFactory("video", FID, {"features_dir": root / "features", "index_dir": sdir})
        assert si2.load_index(itype) is True
        assert type(si2.index) is type(idx) and si2.index.nprobe == 8 and si2.index.local.pos_base == shard_range(N, rank, world)[0]
        out.update({f"{itype}_B_{k}": v for k, v in _collect(si2, d).items()})
        out[f"{itype}_B_list_off"] = si2.index.local.list_off
        # (C) a part is missing on one rank: without a single file every rank refuses; with one every rank reads the single file
        mdir = root / ("index_mixed_" + itype)
        if rank == 0:
            mdir.mkdir()
            shutil.copyfile(part, mdir / part.name)
        dist.barrier()
        si3 = SearchIndexFactory("video", FID, {"features_dir": root / "features", "index_dir": mdir})
        with pytest.raises(RuntimeError, match="never mixed"):
            si3.load_index(itype)
        dist.barrier()
        if rank == 0:
            shutil.copyfile(sdir / si.get_index_filename(itype).name, mdir / si.get_index_filename(itype).name)
        dist.barrier()
        assert si3.load_index(itype) is True
        assert np.array_equal(si3.index.local.list_off, si2.index.local.list_off)        # rank 0 too reads its RANGE, not its part
        D3, I3 = si3.index.search(np.random.default_rng(6).standard_normal((3, d)).astype(np.float32), 25)
        assert np.array_equal(I3, out[f"{itype}_B_I"]) and np.array_equal(D3, out[f"{itype}_B_D"])
    np.savez(root / f"ivfpq_rank{rank}.npz", **out)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_ivfpq_through_the_plugin_surface_world2(tmp_path):
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    from wise_amd.index import faiss_io
    from wise_amd.index.ivf_flat import reference_nlist
    from wise_amd.index.sharded import shard_range

    N, d, m, world = 1001, 32, 8, 2
    X = np.random.default_rng(5).standard_normal((N, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X[700] = X[20]                                                       # equal codes and rows on both ranks' slices
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
    sample = np.sort(np.random.default_rng(1234).permutation(N)[:min(N, 100 * nlist)])
    tower = _FakeTextTower(d)
    q1 = torch.from_numpy(tower.extract_text_features(["This is a photo of a dog"]))
    qb = torch.from_numpy(tower.extract_text_features(["This is a photo of a " + s for s in QUERIES]))
    Q = torch.from_numpy(np.random.default_rng(6).standard_normal((3, d)).astype(np.float32))
    for itype in TYPES:
        kind = {"IndexIVFPQ8": None, "IndexIVFPQ8R8": 8, "IndexIVFPQ8R16": 16}[itype]
        ref = _CpuIVFPQ(d, nlist, m) if kind is None else _CpuIVFPQRefine(d, nlist, m, kind, k_factor=6)
        ref.train(Xcat[sample])
        a, codes, *extra = ref.encode_rows(Xcat)
        order = np.argsort(a, kind="stable")
        off = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=nlist))]).astype(np.int64)
        read = faiss_io.read_ivf_pq_ip if kind is None else faiss_io.read_ivf_pq_refine_ip
        for r in range(world):
            p = read(tmp_path / "index_parts" / f"video-{itype}.faiss.part-{r:03d}-of-{world:03d}")
            lo, hi = shard_range(N, r, world)
            assert p["centroids"].tobytes() == ref.centroids.tobytes() and p["codebooks"].tobytes() == ref.codebooks.tobytes(), r
            assert np.array_equal(p["codes"], codes[order][lo:hi]) and np.array_equal(p["ids"], idcat[order][lo:hi]), r
            assert np.array_equal(p["list_off"], np.clip(off - lo, 0, hi - lo)), r
            if kind is not None:
                assert p["kind"] == kind and np.array_equal(p["rows"].view(np.uint8), extra[0][order][lo:hi].view(np.uint8)), r
                assert p["scales"] is None if kind == 16 else np.array_equal(p["scales"], extra[1][order][lo:hi]), r
        # one single-process stand-in over all rows answers what the collective search answers
        lists = (torch.from_numpy(codes[order]), torch.from_numpy(idcat[order]), torch.from_numpy(off))
        if kind is not None:
            lists += (torch.from_numpy(extra[0][order]), None if kind == 16 else torch.from_numpy(extra[1][order]))
        ref.adopt_lists(*lists)
        ref.nprobe = 8
        D1, I1 = (t.numpy() for t in ref.search_device(q1, 7))
        Db, Ib = (t.numpy() for t in ref.search_device(qb, 9))
        D3, I3 = (t.numpy() for t in ref.search_device(Q, 25))
        assert (I3 >= 0).all() and (I1 >= 0).all()
        rec_ref = ref.reconstruct_batch(WANT_IDS)
        assert np.isfinite(rec_ref[:3]).all() and np.isnan(rec_ref[3]).all()
        for r in range(world):
            g = np.load(tmp_path / f"ivfpq_rank{r}.npz")
            for tag in "AB":
                t = f"{itype}_{tag}_"
                assert np.array_equal(g[t + "ids"], I1[0]) and np.array_equal(g[t + "dist"], D1[0]), (itype, r, tag)
                assert np.array_equal(g[t + "sb_I"], Ib) and np.array_equal(g[t + "sb_D"], Db), (itype, r, tag)
                assert np.array_equal(g[t + "I"], I3) and np.array_equal(g[t + "D"], D3), (itype, r, tag)
                assert np.array_equal(g[t + "rec"], rec_ref, equal_nan=True), (itype, r, tag)
                assert int(g[t + "ntotal"][0]) == N
                # the last search of _collect: nq = 3, k = 25; one exchange, or two (candidates(25) = 150 at k_factor 6)
                assert int(g[t + "xbytes"][0]) == (16 * 3 * 25 if kind is None else 16 * 3 * (150 + 25)), (itype, r, tag)
            lo, hi = shard_range(N, r, world)
            assert np.array_equal(g[f"{itype}_B_list_off"], np.clip(off - lo, 0, hi - lo))

"""CPU tests (-m "not gpu") of IndexIVFSQ8 sharded across ranks (wise_amd/index/sharded.py ShardedIVFSQIPIndex): the ranged reader
of the 'IwSq' file, part files, the declared entry points, and the multi-rank build / load / collective search through the plugin
surface (SearchIndexFactory) at world size 2 over gloo.  A rank's rows live in a numpy stand-in built on tests/ivfsq_ref.py here;
tests/test_gpu_ivfsq_sharded.py runs the HIP kernels and RCCL."""
import os
import re
import shutil
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ivfsq_ref as sq

ROOT = Path(__file__).resolve().parent.parent
FID = "mlfoundations/open_clip/ViT-B-32/seeded-0"
ITYPE = "IndexIVFSQ8"


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ---------------------------------------------------------------------------------------------------------------------
# faiss_io.read_ivf_sq_ip_range / ivf_sq_ip_ntotal / part files
def _sq_file(path, sizes, d, seed):
    from wise_amd.index import faiss_io

    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    n = int(sizes.sum())
    f = {"list_off": np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
         "codes": rng.integers(0, 256, size=(n, d), dtype=np.uint8),
         "ids": rng.permutation(10 * n + 1)[:n].astype(np.int64) + 3,
         "centroids": rng.standard_normal((len(sizes), d)).astype(np.float32),
         "trained": rng.standard_normal(2 * d).astype(np.float32)}
    faiss_io.write_ivf_sq_ip(path, f["centroids"], f["trained"], f["codes"], f["ids"], f["list_off"], nprobe=7)
    return f


@pytest.mark.parametrize("sizes", [
    [5, 0, 0, 17, 1, 0, 9, 0, 0, 0, 3, 12],           # most lists empty ('sprs' layout), lists straddle boundaries
    [40, 3, 8, 2, 11, 6, 1, 4, 9, 2],                 # 'full' layout, one list larger than a rank's share
    [10, 10, 0, 10, 10, 10],                          # W = 2 and 5 cut exactly at list boundaries (one of them beside an empty list)
    [0, 0, 0, 6, 0, 0],                               # one non-empty list: all ranks cut the same list
    [0, 0, 0],                                        # no rows at all: every range is empty
])
def test_range_reader_tiles_the_file(tmp_path, sizes):
    from wise_amd.index import faiss_io
    from wise_amd.index.sharded import shard_range

    fn = tmp_path / "x.faiss"
    d = 16
    w = _sq_file(fn, sizes, d, seed=len(sizes))
    full = faiss_io.read_ivf_sq_ip(fn)
    n = w["codes"].shape[0]
    assert np.array_equal(full["codes"], w["codes"]) and np.array_equal(full["list_off"], w["list_off"])
    assert faiss_io.ivf_sq_ip_ntotal(fn) == n
    for W in (1, 2, 5):
        parts = []
        for r in range(W):
            lo, hi = shard_range(n, r, W)
            p = faiss_io.read_ivf_sq_ip_range(fn, lo, hi)
            assert np.array_equal(p["centroids"], w["centroids"]) and p["nprobe"] == 7
            assert p["trained"].tobytes() == w["trained"].tobytes()
            assert p["codes"].shape == (hi - lo, d) and p["codes"].dtype == np.uint8 and p["ids"].shape == (hi - lo,)
            assert np.array_equal(p["list_off"], np.clip(w["list_off"] - lo, 0, hi - lo)), (W, r)
            assert p["list_off"][0] == 0 and p["list_off"][-1] == hi - lo and (np.diff(p["list_off"]) >= 0).all()
            # a part written with these clipped offsets is a valid small index for the unsharded reader
            pf = tmp_path / f"x.faiss.part-{r:03d}-of-{W:03d}"
            faiss_io.write_ivf_sq_ip(pf, p["centroids"], p["trained"], p["codes"], p["ids"], p["list_off"], nprobe=p["nprobe"])
            back = faiss_io.read_ivf_sq_ip(pf)
            assert faiss_io.index_fourcc(pf) == "IwSq" and faiss_io.ivf_sq_ip_ntotal(pf) == hi - lo
            for key in ("centroids", "codes", "ids", "list_off"):
                assert np.array_equal(back[key], p[key]), (W, r, key)
            assert back["trained"].tobytes() == p["trained"].tobytes() and back["nprobe"] == 7
            parts.append(p)
        for a in ("codes", "ids"):
            assert np.array_equal(np.concatenate([p[a] for p in parts]), full[a]), (W, a)
        assert np.array_equal(sum(p["list_off"] for p in parts), full["list_off"]), W    # the clipped offsets add up
    if n:
        e = faiss_io.read_ivf_sq_ip_range(fn, n // 2, n // 2)                            # an empty range inside the file
        assert e["codes"].shape == (0, d) and not e["list_off"].any()


def test_range_reader_reads_only_the_overlapping_lists(tmp_path, monkeypatch):
    from wise_amd.index import faiss_io

    fn = tmp_path / "x.faiss"
    d = 16
    w = _sq_file(fn, [50, 50, 50, 50], d, seed=1)
    counts = []
    real = np.fromfile
    monkeypatch.setattr(faiss_io.np, "fromfile", lambda *a, **k: counts.append(k.get("count", -1)) or real(*a, **k))
    p = faiss_io.read_ivf_sq_ip_range(fn, 60, 90)                        # inside list 1
    assert np.array_equal(p["codes"], w["codes"][60:90]) and np.array_equal(p["ids"], w["ids"][60:90])
    assert sum(counts) - 4 * d - 2 * d - 4 == 30 * d + 30                # centroids + ranges + list sizes, then the slice alone
    with pytest.raises(ValueError):
        faiss_io.read_ivf_sq_ip_range(fn, 10, 201)
    with pytest.raises(RuntimeError):
        faiss_io.read_ivf_sq_ip_range(tmp_path / "missing.faiss", 0, 1)
    flat = tmp_path / "flat.faiss"
    faiss_io.write_ivf_flat_ip(flat, w["centroids"], np.zeros((200, d), np.float32), w["ids"], w["list_off"])
    with pytest.raises(RuntimeError):
        faiss_io.ivf_sq_ip_ntotal(flat)
    short = tmp_path / "short.faiss"
    short.write_bytes(fn.read_bytes()[:-40])                             # the last list's ids are cut short
    with pytest.raises(RuntimeError, match="cut short"):
        faiss_io.read_ivf_sq_ip_range(short, 150, 200)
    assert np.array_equal(faiss_io.read_ivf_sq_ip_range(short, 0, 150)["codes"], w["codes"][:150])   # the lists before it are whole


def test_the_header_declares_the_local_scan_and_the_export_list_names_it():
    from wise_amd import _lib
    from wise_amd.build import declared_symbols

    header = (ROOT / "include" / "wise_hip.h").read_text()
    assert re.search(r"size_t\s+wise_ivfsq_scan_local_workspace_bytes\(int nq, int nprobe, int k\);", header)
    m = re.search(r"int\s+wise_ivfsq_scan_local\(([^;]*)\);", header)
    assert m and "int64_t pos_base" in m.group(1) and "int32_t* probe_count" in m.group(1)
    assert "(ABI 5, additive) wise_ivfsq_scan on ONE RANK's slice" in header
    exports = declared_symbols()                                          # what build.py writes into the linker's version script
    assert "wise_ivfsq_scan_local" in exports and "wise_ivfsq_scan_local_workspace_bytes" in exports
    assert len(_lib.SIGNATURES["wise_ivfsq_scan_local"][1]) == len(m.group(1).split(",")) == 20
    src = (ROOT / "wise_amd" / "csrc" / "ivf_sq.hip").read_text()
    assert 'extern "C" int wise_ivfsq_scan_local(' in src and 'extern "C" size_t wise_ivfsq_scan_local_workspace_bytes(' in src


# ---------------------------------------------------------------------------------------------------------------------
# the plugin surface at world size 2 (gloo) with a numpy stand-in for IVFSQIPIndex
class _DirectMap:
    def __init__(self):
        self.type = 0


class _CpuIVFSQ:
    """What FeatureSearchIndex.ivfsq_index_factory must offer: train / centroids / trained / set_centroids / set_trained /
    encode_rows / adopt_lists(pos_base) / nprobe / search_local_device / reconstruct_batch (and merge_lists for the wrapper)."""

    def __init__(self, d, nlist):
        self.d, self.nlist, self.device = int(d), int(nlist), torch.device("cpu")
        self.nprobe, self.parallel_mode, self.direct_map = 1, 0, _DirectMap()
        self.centroids = self.trained = None
        self.codes, self.ids, self.list_off, self.pos_base = np.zeros((0, d), np.uint8), np.zeros(0, np.int64), np.zeros(nlist + 1, np.int64), 0

    @property
    def is_trained(self):
        return self.centroids is not None and self.trained is not None

    def train(self, x):
        x = np.asarray(x, np.float64)
        c = x[:self.nlist]                                            # deterministic stand-in for k-means
        self.set_centroids((c / np.linalg.norm(c, axis=1, keepdims=True)).astype(np.float32))
        x = x.astype(np.float32)
        self.set_trained(*sq.train(x - self.centroids[self._assign(x)]))

    def set_centroids(self, c):
        self.centroids = np.array(c, dtype=np.float32)

    def set_trained(self, vmin, vdiff):
        self.trained = np.concatenate([np.asarray(vmin, np.float32), np.asarray(vdiff, np.float32)])

    def _assign(self, x):
        return (np.asarray(x, np.float64) @ self.centroids.astype(np.float64).T).argmax(axis=1).astype(np.int64)

    def encode_rows(self, x):
        x = np.asarray(x, np.float32)
        a = self._assign(x)
        return a, sq.encode(x - self.centroids[a], self.trained[:self.d], self.trained[self.d:])

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

    def search_local_device(self, q, k, probe_count=None, positions=False):
        from oracle import ivf_ref

        Q = q.numpy()
        probes = ivf_ref.coarse_probes(self.centroids, Q, min(self.nprobe, self.nlist))
        coarse = Q.astype(np.float64) @ self.centroids.astype(np.float64).T          # per (query, list): independent of the slice
        bias = np.take_along_axis(coarse, probes, axis=1).astype(np.float32)
        W, q0 = sq.query(Q, self.trained[:self.d], self.trained[self.d:])
        D, I = sq.scan(self.codes, self.list_off, None if positions else self.ids, W, q0, probes, bias, k)
        return torch.from_numpy(D), torch.from_numpy(np.where(I >= 0, I + self.pos_base, -1) if positions else I)

    search_device = search_local_device

    def reconstruct_batch(self, want):
        out = np.full((len(want), self.d), np.nan, np.float32)
        rows = sq.decode_rows(self.codes, self.list_off, self.centroids, self.trained[:self.d], self.trained[self.d:])
        for i, w in enumerate(want):
            hit = np.flatnonzero(self.ids == w)
            if len(hit):
                out[i] = rows[hit[0]]
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


WANT_IDS = [1, 1001, 500, 1006]


def _collect(si, d):
    Q = np.random.default_rng(6).standard_normal((3, d)).astype(np.float32)
    out = {}
    out["dist"], out["ids"] = si.search("video", "dog", topk=7)
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
    from wise_amd.index.selector import IDSelectorRange, SearchParameters
    from wise_amd.index.sharded import NO_SELECTOR, ShardedIVFSQIPIndex, shard_range

    fsi.FeatureSearchIndex.ivfsq_index_factory = _CpuIVFSQ
    fsi.FeatureExtractorFactory = lambda fid: _FakeTextTower(d)
    root = Path(root)
    out = {}
    # (A) the collective build: own store shards -> one part file per rank -> load the part
    si = SearchIndexFactory("video", FID, {"features_dir": root / "features", "index_dir": root / "index_parts"})
    si.create_index(ITYPE)
    part = si.get_index_part_filename(ITYPE, rank, world)
    assert part.exists() and not si.get_index_filename(ITYPE).exists() and faiss_io.index_fourcc(part) == "IwSq"
    dist.barrier()
    assert si.load_index(ITYPE) is True
    idx = si.index
    assert type(idx) is ShardedIVFSQIPIndex and idx.is_trained and idx.d == d and idx.local.pos_base == shard_range(N, rank, world)[0]
    idx.nprobe = 8
    idx.make_direct_map(True)
    assert idx.local.nprobe == 8 and idx.direct_map.type == 2 and idx.hbm_bytes() == idx.local.hbm_bytes() and idx.nlist == idx.local.nlist
    with pytest.raises(NotImplementedError) as e:
        idx.search(np.zeros((1, d), np.float32), 3, params=SearchParameters(sel=IDSelectorRange(0, 10)))
    assert str(e.value) == NO_SELECTOR
    out.update({f"A_{k}": v for k, v in _collect(si, d).items()})
    # (B) rank 0 lays the parts end to end into one file; every rank then loads its range of that file
    sdir = root / "index_single"
    if rank == 0:
        ps = [faiss_io.read_ivf_sq_ip(si.get_index_part_filename(ITYPE, r, world)) for r in range(world)]
        sdir.mkdir()
        cat = lambda a: np.concatenate([p[a] for p in ps])
        faiss_io.write_ivf_sq_ip(sdir / si.get_index_filename(ITYPE).name, ps[0]["centroids"], ps[0]["trained"], cat("codes"), cat("ids"),
                                 sum(p["list_off"] for p in ps), nprobe=8)
    dist.barrier()
    si2 = SearchIndexFactory("video", FID, {"features_dir": root / "features", "index_dir": sdir})
    assert si2.load_index(ITYPE) is True
    assert type(si2.index) is ShardedIVFSQIPIndex and si2.index.nprobe == 8 and si2.index.local.pos_base == shard_range(N, rank, world)[0]
    out.update({f"B_{k}": v for k, v in _collect(si2, d).items()})
    out["B_list_off"] = si2.index.local.list_off
    # (C) a part is missing on one rank: without a single file every rank refuses; with one every rank reads the single file
    mdir = root / "index_mixed"
    if rank == 0:
        mdir.mkdir()
        shutil.copyfile(part, mdir / part.name)
    dist.barrier()
    si3 = SearchIndexFactory("video", FID, {"features_dir": root / "features", "index_dir": mdir})
    with pytest.raises(RuntimeError, match="never mixed"):
        si3.load_index(ITYPE)
    dist.barrier()
    if rank == 0:
        shutil.copyfile(sdir / si.get_index_filename(ITYPE).name, mdir / si.get_index_filename(ITYPE).name)
    dist.barrier()
    assert si3.load_index(ITYPE) is True
    assert np.array_equal(si3.index.local.list_off, si2.index.local.list_off)            # rank 0 too reads its RANGE, not its part
    D3, I3 = si3.index.search(np.random.default_rng(6).standard_normal((3, d)).astype(np.float32), 25)
    assert np.array_equal(I3, out["B_I"]) and np.array_equal(D3, out["B_D"])
    # (D) without the switch nothing changes: rank 0 alone builds the one file, every rank loads all of it
    del os.environ["WISE_SHARDED_IVF"]
    si4 = SearchIndexFactory("video", FID, {"features_dir": root / "features", "index_dir": root / "index_unsharded"})
    fsi.IVFSQIPIndex, real = _CpuIVFSQ, fsi.IVFSQIPIndex

    def lists_host(self):
        return self.centroids, self.trained, self.codes, self.ids, self.list_off

    def add_with_ids(self, x, ids):
        a, codes = self.encode_rows(x)
        order = np.argsort(a, kind="stable")
        off = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=self.nlist))]).astype(np.int64)
        self.adopt_lists(torch.from_numpy(codes[order]), torch.from_numpy(np.asarray(ids, np.int64)[order]), torch.from_numpy(off))

    _CpuIVFSQ.lists_host, _CpuIVFSQ.add_with_ids = lists_host, add_with_ids
    try:
        si4.create_index(ITYPE)
        dist.barrier()
        assert si4.get_index_filename(ITYPE).exists() and not si4.get_index_part_filename(ITYPE, rank, world).exists()
        assert si4.load_index(ITYPE) is True
        assert type(si4.index) is _CpuIVFSQ and si4.index.ntotal == N                      # the whole file, no wrapper
        out["D_codes"], out["D_ids"], out["D_list_off"] = si4.index.codes, si4.index.ids, si4.index.list_off
    finally:
        fsi.IVFSQIPIndex = real
    np.savez(root / f"ivfsq_rank{rank}.npz", **out)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_ivfsq_through_the_plugin_surface_world2(tmp_path):
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    from wise_amd.index import faiss_io
    from wise_amd.index.ivf_flat import reference_nlist
    from wise_amd.index.sharded import shard_range

    N, d, world = 1001, 32, 2
    X = np.random.default_rng(5).standard_normal((N, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X[700] = X[20]                                                       # equal codes on both ranks' slices
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
    ref = _CpuIVFSQ(d, nlist)
    ref.train(Xcat[sample])
    a, codes = ref.encode_rows(Xcat)
    order = np.argsort(a, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=nlist))]).astype(np.int64)
    for r in range(world):
        p = faiss_io.read_ivf_sq_ip(tmp_path / "index_parts" / f"video-{ITYPE}.faiss.part-{r:03d}-of-{world:03d}")
        lo, hi = shard_range(N, r, world)
        assert p["centroids"].tobytes() == ref.centroids.tobytes() and p["trained"].tobytes() == ref.trained.tobytes(), r
        assert np.array_equal(p["codes"], codes[order][lo:hi]) and np.array_equal(p["ids"], idcat[order][lo:hi]), r
        assert np.array_equal(p["list_off"], np.clip(off - lo, 0, hi - lo)), r
    # one single-process stand-in over all rows answers what the collective search answers
    ref.adopt_lists(torch.from_numpy(codes[order]), torch.from_numpy(idcat[order]), torch.from_numpy(off))
    ref.nprobe = 8
    tower = _FakeTextTower(d)
    q1 = torch.from_numpy(tower.extract_text_features(["This is a photo of a dog"]))
    Q = torch.from_numpy(np.random.default_rng(6).standard_normal((3, d)).astype(np.float32))
    D1, I1 = (t.numpy() for t in ref.search_device(q1, 7))
    D3, I3 = (t.numpy() for t in ref.search_device(Q, 25))
    assert (I3 >= 0).all() and (I1 >= 0).all()
    rec_ref = ref.reconstruct_batch(WANT_IDS)
    assert np.isfinite(rec_ref[:3]).all() and np.isnan(rec_ref[3]).all()
    for r in range(world):
        g = np.load(tmp_path / f"ivfsq_rank{r}.npz")
        for tag in "AB":
            assert np.array_equal(g[f"{tag}_ids"], I1[0]) and np.array_equal(g[f"{tag}_dist"], D1[0]), (r, tag)
            assert np.array_equal(g[f"{tag}_I"], I3) and np.array_equal(g[f"{tag}_D"], D3), (r, tag)
            assert np.array_equal(g[f"{tag}_rec"], rec_ref, equal_nan=True), (r, tag)
            assert int(g[f"{tag}_ntotal"][0]) == N
            assert int(g[f"{tag}_xbytes"][0]) == 16 * 3 * 25, (r, tag)        # the last search of _collect: nq = 3, k = 25; one exchange
        lo, hi = shard_range(N, r, world)
        assert np.array_equal(g["B_list_off"], np.clip(off - lo, 0, hi - lo))
    # (D): the one-process build of the same store holds the same lists.  It reads the shard files in turn, the ranks read every
    # second one, so inside a list the rows come in another order: offsets are equal, codes are compared per id, ids per list.  (At
    # world size 1 the two orders coincide and the files are equal byte for byte: tests/sharded_ivfsq_nccl_worker.py.)
    g = np.load(tmp_path / "ivfsq_rank1.npz")
    assert np.array_equal(g["D_list_off"], off)
    assert np.array_equal(g["D_codes"][np.argsort(g["D_ids"])], codes[order][np.argsort(idcat[order])])
    for l in range(nlist):
        assert np.array_equal(np.sort(g["D_ids"][off[l]:off[l + 1]]), np.sort(idcat[order][off[l]:off[l + 1]]))

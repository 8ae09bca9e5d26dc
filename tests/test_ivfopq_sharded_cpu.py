"""CPU tests (-m "not gpu") of IndexIVFOPQ<m> / IndexIVFOPQ<m>R8 / R16 sharded across ranks: the multi-rank build / load /
collective search through the plugin surface (SearchIndexFactory) at world size 2 over gloo, with the numpy stand-ins of
tests/test_ivfpq_sharded_cpu.py put behind a rotation (tests/ivfopq_ref.py).  The sharded classes are the IndexIVFPQ ones; what
is new is that rank 0 trains a rotation, that it travels with the codebooks and into every part file, and that every rank
rotates its own rows and the query.  tests/test_gpu_ivfopq_sharded.py runs the HIP kernels and RCCL."""
import os
import sys
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ivfopq_ref
import ivfpq_ref
from test_ivfpq_sharded_cpu import FID, QUERIES, WANT_IDS, _collect, _CpuIVFPQ, _CpuIVFPQRefine, _FakeTextTower, _free_port

ROOT = Path(__file__).resolve().parent.parent
TYPES = ("IndexIVFOPQ8", "IndexIVFOPQ8R8", "IndexIVFOPQ8R16")


class _Rotation:
    """What turns the stand-ins into what FeatureSearchIndex.ivfopq_index_factory / ivfopq_refine_index_factory must offer:
    rotation / set_rotation, codes from the rotated residuals, tables from the rotated queries."""
    rotation = None

    @property
    def is_trained(self):
        return super().is_trained and self.rotation is not None

    def train(self, x):
        x = np.asarray(x, np.float64)
        c = x[:self.nlist]
        self.set_centroids((c / np.linalg.norm(c, axis=1, keepdims=True)).astype(np.float32))
        x = x[:512].astype(np.float32)
        R, cb, _ = ivfopq_ref.train(x - self.centroids[self._assign(x)], self.m, niter=2, opq_niter=2, opq_niter_pq=1)
        self.set_rotation(R.astype(np.float32))
        self.set_codebooks(cb.astype(np.float32))

    def set_rotation(self, R):
        self.rotation = np.array(R, dtype=np.float32)
        assert self.rotation.shape == (self.d, self.d)

    def _rot(self, x):
        return ivfopq_ref.rotate(x, self.rotation).astype(np.float32)

    def encode_rows(self, x):
        x = np.asarray(x, np.float32)
        a = self._assign(x)
        return (a, ivfpq_ref.encode(self._rot(x - self.centroids[a]), self.codebooks), *self._extra(x))

    def _scan(self, Q, k, positions):
        from oracle import ivf_ref

        probes = ivf_ref.coarse_probes(self.centroids, Q, min(self.nprobe, self.nlist))
        coarse = Q.astype(np.float64) @ self.centroids.astype(np.float64).T
        bias = np.take_along_axis(coarse, probes, axis=1).astype(np.float32)
        lut = ivfpq_ref.lut(self._rot(Q), self.codebooks).astype(np.float32)
        D, I = ivfpq_ref.scan(self.codes, self.list_off, None if positions else self.ids, lut, probes, bias, k)
        return D, (np.where(I >= 0, I + self.pos_base, -1) if positions else I)


class _CpuIVFOPQ(_Rotation, _CpuIVFPQ):
    def _row(self, pos, lists):
        cw = ivfopq_ref.codewords(self.codes[pos], self.codebooks)
        return (self.centroids[lists[pos]] + cw @ self.rotation.astype(np.float64)).astype(np.float32)     # c_l + R^T cw


class _CpuIVFOPQRefine(_Rotation, _CpuIVFPQRefine):
    pass


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

    fsi.FeatureSearchIndex.ivfopq_index_factory = _CpuIVFOPQ
    fsi.FeatureSearchIndex.ivfopq_refine_index_factory = _CpuIVFOPQRefine
    fsi.FeatureExtractorFactory = lambda fid: _FakeTextTower(d)
    root = Path(root)
    out = {}
    for itype in TYPES:
        refine = itype != TYPES[0]
        # (A) the collective build: own store shards -> one part file per rank -> load the part
        si = SearchIndexFactory("video", FID, {"features_dir": root / "features", "index_dir": root / "index_parts"})
        si.create_index(itype)
        part = si.get_index_part_filename(itype, rank, world)
        assert part.exists() and not si.get_index_filename(itype).exists() and faiss_io.index_fourcc(part) == "WiOP"
        dist.barrier()
        assert si.load_index(itype) is True
        idx = si.index
        assert type(idx) is (ShardedIVFPQRefineIPIndex if refine else ShardedIVFPQIPIndex)       # the same wrappers ...
        assert type(idx.local) is (_CpuIVFOPQRefine if refine else _CpuIVFOPQ)                    # ... around the rotating classes
        assert idx.is_trained and idx.d == d and idx.local.pos_base == shard_range(N, rank, world)[0]
        idx.nprobe = 8
        if refine:
            idx.k_factor = 6
        out.update({f"{itype}_A_{k}": v for k, v in _collect(si, d).items()})
        # (B) rank 0 lays the parts end to end into one 'WiOP' file; every rank then loads its range of that file
        sdir = root / ("index_single_" + itype)
        if rank == 0:
            ps = [faiss_io.read_ivf_opq_ip(si.get_index_part_filename(itype, r, world)) for r in range(world)]
            assert all(np.array_equal(p["rotation"], ps[0]["rotation"]) for p in ps)
            sdir.mkdir()
            cat = lambda a: np.concatenate([p[a] for p in ps])
            store = dict(kind=ps[0]["kind"], k_factor=6, rows=cat("rows"), scales=None if ps[0]["scales"] is None else cat("scales")) if refine else {}
            faiss_io.write_ivf_opq_ip(sdir / si.get_index_filename(itype).name, ps[0]["rotation"], ps[0]["centroids"], ps[0]["codebooks"],
                                      cat("codes"), cat("ids"), sum(p["list_off"] for p in ps), nprobe=8, **store)
        dist.barrier()
        si2 = SearchIndexFactory("video", FID, {"features_dir": root / "features", "index_dir": sdir})
        assert si2.load_index(itype) is True
        assert type(si2.index) is type(idx) and si2.index.nprobe == 8 and si2.index.local.pos_base == shard_range(N, rank, world)[0]
        assert np.array_equal(si2.index.local.rotation, idx.local.rotation)
        out.update({f"{itype}_B_{k}": v for k, v in _collect(si2, d).items()})
        out[f"{itype}_B_list_off"] = si2.index.local.list_off
    np.savez(root / f"ivfopq_rank{rank}.npz", **out)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_ivfopq_through_the_plugin_surface_world2(tmp_path):
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

    rows, rids = [], []
    for r in range(world):                                               # every rank's store rows, in rank order
        rd = FeatureStoreFactory.load_store("video", fdir)
        rd.enable_read(shard_shuffle=False, shard_slice=(r, world))
        for fids, vecs in rd.iter_batch():
            rows.append(np.asarray(vecs, np.float32))
            rids.append(np.asarray(fids, np.int64))
    Xcat, idcat = np.concatenate(rows), np.concatenate(rids)
    nlist = reference_nlist(N)
    sample = np.sort(np.random.default_rng(1234).permutation(N)[:min(N, 100 * nlist)])
    tower = _FakeTextTower(d)
    q1 = torch.from_numpy(tower.extract_text_features(["This is a photo of a dog"]))
    qb = torch.from_numpy(tower.extract_text_features(["This is a photo of a " + s for s in QUERIES]))
    Q = torch.from_numpy(np.random.default_rng(6).standard_normal((3, d)).astype(np.float32))
    for itype in TYPES:
        kind = {"IndexIVFOPQ8": None, "IndexIVFOPQ8R8": 8, "IndexIVFOPQ8R16": 16}[itype]
        ref = _CpuIVFOPQ(d, nlist, m) if kind is None else _CpuIVFOPQRefine(d, nlist, m, kind, k_factor=6)
        ref.train(Xcat[sample])
        assert np.abs(ref.rotation - np.eye(d)).max() > 1e-3             # a rotation that does something
        a, codes, *extra = ref.encode_rows(Xcat)
        order = np.argsort(a, kind="stable")
        off = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=nlist))]).astype(np.int64)
        # the parts laid end to end are the single build: rank 0's rotation, centroids and codebooks in every part
        for r in range(world):
            p = faiss_io.read_ivf_opq_ip(tmp_path / "index_parts" / f"video-{itype}.faiss.part-{r:03d}-of-{world:03d}")
            lo, hi = shard_range(N, r, world)
            assert p["rotation"].tobytes() == ref.rotation.tobytes(), r
            assert p["centroids"].tobytes() == ref.centroids.tobytes() and p["codebooks"].tobytes() == ref.codebooks.tobytes(), r
            assert np.array_equal(p["codes"], codes[order][lo:hi]) and np.array_equal(p["ids"], idcat[order][lo:hi]), r
            assert np.array_equal(p["list_off"], np.clip(off - lo, 0, hi - lo)), r
            assert ("kind" in p) == (kind is not None)
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
            g = np.load(tmp_path / f"ivfopq_rank{r}.npz")
            for tag in "AB":
                t = f"{itype}_{tag}_"
                assert np.array_equal(g[t + "ids"], I1[0]) and np.array_equal(g[t + "dist"], D1[0]), (itype, r, tag)
                assert np.array_equal(g[t + "sb_I"], Ib) and np.array_equal(g[t + "sb_D"], Db), (itype, r, tag)
                assert np.array_equal(g[t + "I"], I3) and np.array_equal(g[t + "D"], D3), (itype, r, tag)
                assert np.array_equal(g[t + "rec"], rec_ref, equal_nan=True), (itype, r, tag)
                assert int(g[t + "ntotal"][0]) == N
                # no extra exchange for the rotation: one exchange, or two (candidates(25) = 150 at k_factor 6), as IndexIVFPQ
                assert int(g[t + "xbytes"][0]) == (16 * 3 * 25 if kind is None else 16 * 3 * (150 + 25)), (itype, r, tag)
            lo, hi = shard_range(N, r, world)
            assert np.array_equal(g[f"{itype}_B_list_off"], np.clip(off - lo, 0, hi - lo))

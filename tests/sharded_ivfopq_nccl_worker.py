"""Worker of tests/test_gpu_ivfopq_sharded.py (not a test module): ONE rank on the `nccl` backend (= RCCL) on the GPU box.

Initialises the process group before any other GPU call, then drives the sharded IndexIVFOPQ16 / IndexIVFOPQ16R8 /
IndexIVFOPQ16R16 through the plugin surface with WISE_SHARDED_INDEX=1 WISE_SHARDED_IVF=1: create_index (the collective build:
sample, train, broadcast of centroids, codebooks AND the rotation, rotate + encode, all-gather of list counts, all_to_all of
codes and compact rows) writes part-000-of-001 — a complete 'WiOP' file — load_index gives the IndexIVFPQ sharded wrapper around
the rotating local class, whose all-gathers and wise_topk_merge really run, and every answer is compared bit for bit with the
unsharded index over the same state.  Prints one JSON line."""
import json
import os
import shutil
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main(tmp):
    import numpy as np
    import torch
    import torch.distributed as dist

    os.environ["WISE_SHARDED_INDEX"] = "1"
    os.environ["WISE_SHARDED_IVF"] = "1"
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    from wise_amd.index import faiss_io
    from wise_amd.index.ivf_pq import IVFOPQIPIndex, IVFOPQRefineIPIndex
    from wise_amd.index.search_index_factory import SearchIndexFactory
    from wise_amd.index.sharded import ShardedIVFPQIPIndex, ShardedIVFPQRefineIPIndex

    tmp = Path(tmp)
    fid = "mlfoundations/open_clip/ViT-B-32/seeded-0"
    res = {"exchange_bytes": {}}
    N, d = 20000, 512
    X = np.random.default_rng(2).standard_normal((N, d), dtype=np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X[15000] = X[3]                                                     # two rows with equal codes and equal compact rows
    (tmp / "features").mkdir()
    st = FeatureStoreFactory.create_store(FeatureStoreType.NUMPY, "video", str(tmp / "features"))
    st.enable_write(4000, 0)
    for i in range(N):
        st.add(i + 1, X[i:i + 1])
    st.close()
    Q = np.random.default_rng(3).standard_normal((4, d)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    Q[1] = X[3]
    ok = True
    for itype in ("IndexIVFOPQ16", "IndexIVFOPQ16R8", "IndexIVFOPQ16R16"):
        refine = itype != "IndexIVFOPQ16"
        si = SearchIndexFactory("video", fid, {"features_dir": tmp / "features", "index_dir": tmp / "index"})
        si.create_index(itype)
        part = si.get_index_part_filename(itype, 0, 1)
        good = part.exists() and not si.get_index_filename(itype).exists()
        assert si.load_index(itype) is True
        idx = si.index
        assert type(idx) is (ShardedIVFPQRefineIPIndex if refine else ShardedIVFPQIPIndex) and idx.always_exchange and idx.world == 1
        assert dist.get_backend() == "nccl" and idx.local.pos_base == 0 and idx.is_trained
        assert type(idx.local) is (IVFOPQRefineIPIndex if refine else IVFOPQIPIndex) and faiss_io.index_fourcc(part) == "WiOP"
        good &= idx.ntotal == N and idx.nlist == idx.local.nlist and idx.hbm_bytes() == idx.local.hbm_bytes()   # all_reduce over RCCL
        # the unsharded index over a single file of the same lists (what load_index builds outside a process group)
        single = tmp / ("single-" + itype + ".faiss")
        shutil.copyfile(part, single)
        f = faiss_io.read_ivf_opq_ip(single)
        nlist, m = f["centroids"].shape[0], f["codebooks"].shape[0]
        lists = (torch.from_numpy(f["codes"]), torch.from_numpy(f["ids"]), torch.from_numpy(f["list_off"]))
        if refine:
            plain = IVFOPQRefineIPIndex(d, nlist, m, f["kind"], k_factor=f["k_factor"])
            lists += (torch.from_numpy(f["rows"] if f["kind"] == 8 else f["rows"].view(np.int16)),
                      None if f["scales"] is None else torch.from_numpy(f["scales"]))
        else:
            plain = IVFOPQIPIndex(d, nlist, m)
        plain.set_centroids(f["centroids"])
        plain.set_codebooks(f["codebooks"])
        plain.set_rotation(f["rotation"])
        good &= bool(torch.equal(plain.rotation, idx.local.rotation))
        res[itype + "_rotation_off_identity"] = float((plain.rotation - torch.eye(d, device="cuda")).abs().max())
        plain.adopt_lists(*lists)
        assert plain.ntotal == N and m == 16
        good &= bool(np.array_equal(np.sort(f["ids"]), np.arange(1, N + 1)) and f["list_off"][-1] == N)
        if refine:
            idx.k_factor = plain.k_factor = 50
            res["candidates"] = idx.local.candidates(10)
        for nprobe, nq, k in [(1, 1, 10), (32, 4, 20), (128, 2, 1000), (idx.nlist, 4, 10), (16, 3, 100), (16, 3, 10)]:
            idx.nprobe = nprobe
            plain.nprobe = nprobe
            D, I = idx.search(Q[:nq], k)                                # all_gather_into_tensor + wise_topk_merge (twice for R8 / R16)
            Dp, Ip = plain.search(Q[:nq], k)
            same = bool(idx.local.nprobe == nprobe and np.array_equal(I, Ip) and np.array_equal(D.view(np.int32), Dp.view(np.int32))
                        and (I[:, 0] >= 0).all())
            res[f"{itype}_np{nprobe}_nq{nq}_k{k}"] = same
            good &= same
        res["exchange_bytes"][itype] = idx.last_exchange_bytes          # of the last search: nq = 3, k = 10
        want = np.array([1, 15001, N + 3], dtype=np.int64)
        rec, recp = idx.reconstruct_batch(want), plain.reconstruct_batch(want)
        good &= bool(np.array_equal(rec[:2], recp[:2]) and np.isnan(rec[2]).all() and np.isfinite(rec[:2]).all())
        res[itype] = bool(good)
        ok &= bool(good)
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()
    res["ok"] = bool(ok)
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1])

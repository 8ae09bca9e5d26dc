"""Worker of tests/test_gpu_ivf_l2_sharded.py (not a test module): ONE rank on the `nccl` backend (= RCCL) on the GPU box.

Initialises the process group before any other GPU call, then drives IndexIVFFlatL2 through the plugin surface twice over the same
feature store.  With WISE_SHARDED_INDEX=1 WISE_SHARDED_IVF=1, create_index (the collective build: sample, train, broadcast of
the centroids, assign, all-gather of list counts, all_to_all of the fp32 rows) writes part-000-of-001 and load_index gives the
sharded wrapper whose all-gather and wise_topk_merge really run, on negated distances.  With WISE_SHARDED_IVF unset the same two
calls are the unsharded plugin: rank 0 builds the single file, load_index gives an IVFFlatL2Index.  The part must be the single file
byte for byte, and every answer of the wrapper the unsharded answer's bits.  Prints one JSON line."""
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main(tmp):
    import numpy as np
    import torch
    import torch.distributed as dist

    os.environ["WISE_SHARDED_INDEX"] = "1"
    os.environ["WISE_SHARDED_IVF"] = "1"
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    import ivf_l2_ref
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    from wise_amd.index import faiss_io
    from wise_amd.index.ivf_flat import IVFFlatL2Index
    from wise_amd.index.search_index_factory import SearchIndexFactory
    from wise_amd.index.selector import IDSelectorRange, SearchParameters
    from wise_amd.index.sharded import ShardedIVFFlatIPIndex

    tmp = Path(tmp)
    fid = "mlfoundations/open_clip/ViT-B-32/seeded-0"
    itype = "IndexIVFFlatL2"
    res = {}
    N, d = 4096, 64
    X = ivf_l2_ref.long_rows(N, d, 21, centres=16)               # lengths spread over 4x, not normalised
    X[3000] = X[3]                                                      # two equal rows
    (tmp / "features").mkdir()
    st = FeatureStoreFactory.create_store(FeatureStoreType.NUMPY, "video", str(tmp / "features"))
    st.enable_write(1000, 0)
    for i in range(N):
        st.add(i + 1, X[i:i + 1])
    st.close()
    Q = ivf_l2_ref.long_rows(4, d, 3)
    Q[1] = X[3]

    si = SearchIndexFactory("video", fid, {"features_dir": tmp / "features", "index_dir": tmp / "index"})
    si.create_index(itype)
    part = si.get_index_part_filename(itype, 0, 1)
    good = part.exists() and not si.get_index_filename(itype).exists() and faiss_io.index_fourcc(part) == "IwFl" and faiss_io.ivf_flat_metric(part) == 1
    assert si.load_index(itype) is True
    idx = si.index
    assert type(idx) is ShardedIVFFlatIPIndex and type(idx.local) is IVFFlatL2Index and idx.always_exchange and idx.world == 1
    assert dist.get_backend() == "nccl" and idx.local.pos_base == 0 and idx.is_trained
    good &= idx.ntotal == N and idx.nlist == idx.local.nlist and idx.local.metric == "l2"   # all_reduce over RCCL
    res["part"] = bool(good)

    # the unsharded plugin over the same store: without the switch rank 0 builds the one file and load_index gives the plain index
    del os.environ["WISE_SHARDED_IVF"]
    sp = SearchIndexFactory("video", fid, {"features_dir": tmp / "features", "index_dir": tmp / "index-single"})
    sp.create_index(itype)
    single = sp.get_index_filename(itype)
    assert single.exists() and not sp.get_index_part_filename(itype, 0, 1).exists()
    assert sp.load_index(itype) is True
    plain = sp.index
    assert type(plain) is IVFFlatL2Index and plain.ntotal == N
    os.environ["WISE_SHARDED_IVF"] = "1"
    f = faiss_io.read_index(part)
    same_file = part.read_bytes() == single.read_bytes() and f["X"].dtype == np.float32 and f["metric"] == "l2"
    same_file &= bool(np.array_equal(np.sort(f["ids"]), np.arange(1, N + 1)) and f["list_off"][-1] == N)
    res["same_file"] = bool(same_file)                                  # the part IS the one-process build, byte for byte
    good &= same_file

    for nprobe, nq, k in [(1, 1, 10), (8, 4, 20), (idx.nlist, 2, 1000), (idx.nlist, 4, 10), (16, 3, 100), (16, 3, 10)]:
        idx.nprobe = nprobe
        plain.nprobe = nprobe
        D, I = idx.search(Q[:nq], k)                                    # all_gather_into_tensor + wise_topk_merge
        Dp, Ip = plain.search(Q[:nq], k)
        same = bool(idx.local.nprobe == nprobe and np.array_equal(I, Ip) and np.array_equal(D.view(np.int32), Dp.view(np.int32))
                    and (I[:, 0] >= 0).all())
        res[f"np{nprobe}_nq{nq}_k{k}"] = same
        good &= same
    res["exchange_bytes"] = idx.last_exchange_bytes                     # of the last search: nq = 3, k = 10
    idx.nprobe = plain.nprobe = idx.nlist
    D, I = idx.search(Q[1:2], 10)                                       # the two equal rows: distance 0 twice, list order kept
    good &= bool(set(I[0, :2]) == {4, 3001} and D[0, 0] == D[0, 1] == 0 and D[0, 2] > 0 and (np.diff(D[0]) >= 0).all())
    Dp, Ip = plain.search(Q[1:2], 10)
    good &= bool(np.array_equal(I, Ip))
    want = np.array([1, 3001, N + 3], dtype=np.int64)
    rec, recp = idx.reconstruct_batch(want), plain.reconstruct_batch(want)
    good &= bool(np.array_equal(rec[:2].view(np.int32), recp[:2].view(np.int32)) and np.isnan(rec[2]).all() and np.array_equal(rec[:2], X[[0, 3000]]))
    try:
        idx.search(Q[:1], 5, params=SearchParameters(sel=IDSelectorRange(0, 10)))
        good = False                                                    # a selector must be refused
    except NotImplementedError:
        pass
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()
    res["ok"] = bool(good)
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1])

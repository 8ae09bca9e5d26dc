"""Worker of tests/test_gpu_ivf_sharded.py (not a test module): ONE rank on the `nccl` backend (= RCCL) on the GPU box.

Initialises the process group before any other GPU call, then drives the sharded IndexIVFFlat through the plugin surface
with WISE_SHARDED_INDEX=1 WISE_SHARDED_IVF=1: create_index (the collective build: sample, train, broadcast, assign,
all-gather of list counts, all_to_all of rows) writes part-000-of-001, load_index gives a ShardedIVFFlatIPIndex whose
all-gather and wise_topk_merge really run, and every answer is compared bit for bit with the unsharded IVFFlatIPIndex
built from the same centroids and rows.  Prints one JSON line."""
import json
import os
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
    from wise_amd.index.ivf_flat import IVFFlatIPIndex, reference_nlist
    from wise_amd.index.search_index_factory import SearchIndexFactory
    from wise_amd.index.sharded import ShardedIVFFlatIPIndex

    tmp = Path(tmp)
    fid = "mlfoundations/open_clip/ViT-B-32/seeded-0"
    res = {}
    N, d = 20000, 512
    X = np.random.default_rng(2).standard_normal((N, d), dtype=np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X[15000] = X[3]                                                     # two rows with equal scores
    (tmp / "features").mkdir()
    st = FeatureStoreFactory.create_store(FeatureStoreType.NUMPY, "video", str(tmp / "features"))
    st.enable_write(4000, 0)
    for i in range(N):
        st.add(i + 1, X[i:i + 1])
    st.close()
    si = SearchIndexFactory("video", fid, {"features_dir": tmp / "features", "index_dir": tmp / "index"})
    si.create_index("IndexIVFFlat")
    part = si.get_index_part_filename("IndexIVFFlat", 0, 1)
    res["part_file"] = part.exists() and not si.get_index_filename("IndexIVFFlat").exists()
    assert si.load_index("IndexIVFFlat") is True
    idx = si.index
    assert isinstance(idx, ShardedIVFFlatIPIndex) and idx.always_exchange and idx.world == 1
    assert dist.get_backend() == "nccl"
    res["ntotal"] = idx.ntotal                                          # all_reduce over RCCL
    # the unsharded index from the same centroids and the same rows (added in store order)
    f = faiss_io.read_ivf_flat_ip(part)
    nlist = reference_nlist(N)
    plain = IVFFlatIPIndex(d, nlist)
    plain.set_centroids(f["centroids"])
    rd = FeatureStoreFactory.load_store("video", tmp / "features")
    rd.enable_read(shard_shuffle=False)
    for fids, vecs in rd.iter_batch():
        plain.add_with_ids(np.asarray(vecs, np.float32), np.asarray(fids, np.int64))
    c, Xs, ids_s, off = plain.lists_host()
    res["lists"] = bool(f["centroids"].shape == (nlist, d) and np.array_equal(Xs, f["X"])
                        and np.array_equal(ids_s, f["ids"]) and np.array_equal(off, f["list_off"]))
    idx.parallel_mode = 1
    idx.make_direct_map(True)
    Q = np.random.default_rng(3).standard_normal((4, d)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    Q[1] = X[3]
    ok = True
    for nprobe, nq, k in [(1, 1, 10), (32, 4, 20), (128, 2, 1000), (nlist, 4, 10), (16, 3, 100)]:
        idx.nprobe = nprobe
        plain.nprobe = nprobe
        D, I = idx.search(Q[:nq], k)                                    # all_gather_into_tensor + wise_topk_merge
        Dp, Ip = plain.search(Q[:nq], k)
        same = bool(idx.local.nprobe == nprobe and np.array_equal(I, Ip) and np.array_equal(D.view(np.int32), Dp.view(np.int32)))
        res[f"search_np{nprobe}_nq{nq}_k{k}"] = same
        ok &= same
    res["exchange_bytes"] = idx.last_exchange_bytes
    rec = idx.reconstruct_batch(np.array([1, 15001, N + 3], dtype=np.int64))
    res["reconstruct"] = bool(np.array_equal(rec[0], X[0]) and np.array_equal(rec[1], X[15000]) and np.isnan(rec[2]).all())
    idx.nprobe = plain.nprobe = 32
    texts = ["dog", "cat", "a red car"]
    got = si.search_batch("video", texts, topk=7)
    feats = si.feature_extractor.extract_text_features(["This is a photo of a " + t for t in texts])
    Dp, Ip = plain.search(feats, 7)
    res["search_batch"] = bool(all(np.array_equal(g[1], Ip[i]) and np.array_equal(g[0], Dp[i]) for i, g in enumerate(got)))
    dist_, ids_ = si.search("video", "dog", topk=5)                    # one prompt: a text-tower batch of its own
    Dp, Ip = plain.search(si.feature_extractor.extract_text_features(["This is a photo of a dog"]), 5)
    res["plugin_search"] = bool(np.array_equal(ids_, Ip[0]) and np.array_equal(dist_, Dp[0]))
    idx.nprobe = 16
    idx.search(Q[:3], 100)                                              # the exchange the test pins
    res["exchange_bytes"] = idx.last_exchange_bytes
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()
    res["ok"] = bool(ok and res["part_file"] and res["lists"] and res["reconstruct"] and res["search_batch"]
                     and res["plugin_search"] and res["ntotal"] == N)
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1])

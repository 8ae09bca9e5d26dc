"""Worker of tests/test_gpu_sqfp16_l2.py (not a test module): ONE rank on the `nccl` backend (= RCCL) on the GPU box.

Initialises the process group before any other GPU call, then drives IndexSQfp16L2 through the plugin surface twice over the same
feature store.  With WISE_SHARDED_INDEX=1, create_index writes the rank's part (part-000-of-001, built from the rank's own store
shards) and load_index gives a ShardedFlatIPIndex around a FlatSQfp16L2Index whose all-gather and wise_topk_merge really run — on the
negated distances.  With the switch unset the same two calls are the unsharded plugin: the single file and the plain index.  The
part must be the single file byte for byte, and every answer of the wrapper the unsharded answer's bits.  Prints one JSON line."""
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
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    import sqfp16_l2_ref as ref
    from wise_amd.feature.store.feature_store_factory import FeatureStoreFactory, FeatureStoreType
    from wise_amd.index import faiss_io
    from wise_amd.index.flat_sq import FlatSQfp16L2Index
    from wise_amd.index.search_index_factory import SearchIndexFactory
    from wise_amd.index.selector import IDSelectorRange, SearchParameters
    from wise_amd.index.sharded import ShardedFlatIPIndex

    tmp = Path(tmp)
    fid = "mlfoundations/open_clip/ViT-B-32/seeded-0"
    itype = "IndexSQfp16L2"
    res = {}
    N, d = 4096, 64
    rng = np.random.default_rng(21)
    X = (rng.standard_normal((N, d)) * rng.uniform(0.2, 3.0, size=(N, 1))).astype(np.float32)    # rows that are NOT normalised
    X[3000] = X[3]                                                      # two equal rows
    (tmp / "features").mkdir()
    st = FeatureStoreFactory.create_store(FeatureStoreType.NUMPY, "video", str(tmp / "features"))
    st.enable_write(1000, 0)
    for i in range(N):
        st.add(i + 1, X[i:i + 1])
    st.close()
    Q = rng.standard_normal((4, d)).astype(np.float32)
    Q[1] = X[3].astype(np.float16).astype(np.float32) + np.float32(1e-3) * Q[1]

    si = SearchIndexFactory("video", fid, {"features_dir": tmp / "features", "index_dir": tmp / "index"})
    si.create_index(itype)
    part = si.get_index_part_filename(itype, 0, 1)
    good = part.exists() and not si.get_index_filename(itype).exists() and faiss_io.index_fourcc(part, inner=True) == "IxSQ" and faiss_io.flat_sq_metric(part) == 1
    assert si.load_index(itype) is True
    idx = si.index
    assert type(idx) is ShardedFlatIPIndex and type(idx.local) is FlatSQfp16L2Index and idx.always_exchange and idx.world == 1
    assert dist.get_backend() == "nccl"
    good &= idx.ntotal == N and idx.local.hbm_bytes() == N * (2 * d + 8)   # all_reduce over RCCL
    res["part"] = bool(good)

    # the unsharded plugin over the same store
    del os.environ["WISE_SHARDED_INDEX"]
    sp = SearchIndexFactory("video", fid, {"features_dir": tmp / "features", "index_dir": tmp / "index-single"})
    sp.create_index(itype)
    single = sp.get_index_filename(itype)
    assert single.exists() and not sp.get_index_part_filename(itype, 0, 1).exists()
    assert sp.load_index(itype) is True
    plain = sp.index
    assert type(plain) is FlatSQfp16L2Index and plain.ntotal == N
    os.environ["WISE_SHARDED_INDEX"] = "1"
    H = ref.encode(X)                                                   # what the file and HBM hold: the rows rounded to binary16
    Hf, ids = faiss_io.read_idmap_sq16_l2(part)
    same_file = part.read_bytes() == single.read_bytes() and Hf.dtype == np.float16 and Hf.tobytes() == H.tobytes()
    same_file &= bool(np.array_equal(ids, np.arange(1, N + 1)))
    res["same_file"] = bool(same_file)
    good &= same_file

    for nq, k in [(1, 10), (4, 20), (2, 1000), (3, 100), (3, 10)]:
        D, I = idx.search(Q[:nq], k)                                    # all_gather_into_tensor + wise_topk_merge
        Dp, Ip = plain.search(Q[:nq], k)
        Dr, Ir = ref.topk(H, Q[:nq], k, ids=ids)
        same = bool(np.array_equal(I, Ip) and np.array_equal(D.view(np.int32), Dp.view(np.int32)) and (I[:, 0] >= 0).all()
                    and np.array_equal(I, Ir) and np.array_equal(D.view(np.int32), Dr.view(np.int32)) and (np.diff(D, axis=1) >= 0).all())
        res[f"nq{nq}_k{k}"] = same
        good &= same
    res["exchange_bytes"] = idx.last_exchange_bytes                     # of the last search: nq = 3, k = 10
    D, I = idx.search(Q[1:2], 10)                                       # the two equal rows: equal distances, the lower position first
    good &= bool(I[0, 0] == 4 and I[0, 1] == 3001 and D[0, 0] == D[0, 1])
    want = np.array([1, 3001, N + 3], dtype=np.int64)
    rec, recp = idx.reconstruct_batch(want), plain.reconstruct_batch(want)
    good &= bool(np.array_equal(rec[:2].view(np.int32), recp[:2].view(np.int32)) and np.isnan(rec[2]).all() and np.isfinite(rec[:2]).all())
    good &= bool(np.array_equal(rec[:2], H[[0, 3000]].astype(np.float32)))
    res["wrapper_answers"] = bool(good)
    # the plugin's own calls on the unsharded index: search, within, search_range
    calls = True

    class Tower:
        def extract_text_features(self, texts):
            return Q[2:3]
    sp.feature_extractor = Tower()
    dist_, ids_ = sp.search("video", "dog", topk=7)
    Dr, Ir = ref.topk(H, Q[2:3], 7, ids=ids)
    calls &= bool(np.array_equal(ids_, Ir[0]) and np.array_equal(dist_.view(np.int32), Dr[0].view(np.int32)))
    dw, iw = sp.search("video", "dog", topk=7, within=np.arange(100, 900))
    Dw, Iw = ref.topk_pos(H, Q[2:3], 7, np.arange(99, 899), ids=ids)
    calls &= bool(np.array_equal(iw, Iw[0]) and np.array_equal(dw.view(np.int32), Dw[0].view(np.int32)))
    radius = float(Dr[0, 6])
    dr, ir = sp.search_range("video", "dog", radius)
    calls &= bool(np.array_equal(ir, Ir[0, :len(ir)]) and len(ir) == int((Dr[0] < radius).sum()) and len(ir) > 0)
    res["plugin_calls"] = bool(calls)
    good &= calls
    for refused in (lambda: idx.search(Q[:1], 5, params=SearchParameters(sel=IDSelectorRange(0, 10))), lambda: idx.range_search(Q[:1], 0.5),
                    lambda: idx.remove_ids(np.array([1]))):
        try:
            refused()
            good = False                                                # the sharded wrapper's refusals stay
        except NotImplementedError:
            pass
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()
    res["ok"] = bool(good)
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1])

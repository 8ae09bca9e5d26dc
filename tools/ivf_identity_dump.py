"""Everything an IndexIVFFlat and an IndexIVFPQ<m> compute from fixed seeds, written to one .npz: run it on two commits on
the same GPU and compare the files array by array (`--compare A B`: bytes, so NaN-safe).  Public methods only.

For d in {64, 512}: train, add_with_ids, search, add_with_ids again (so old and pending lists are merged), then `centroids`,
`lists_host()`, `search_device` and `search_local_device` (with `probe_count`) at nprobe in {8, 128} and nq in {1, 256},
k = 10, and `reconstruct_batch` of known and unknown ids.

    timeout 300 python tools/ivf_identity_dump.py --out FILE.npz
    python tools/ivf_identity_dump.py --compare A.npz B.npz
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def dump(out):
    import torch

    from wise_amd.index.ivf_flat import IVFFlatIPIndex
    from wise_amd.index.ivf_pq import IVFPQIPIndex

    arrays, k = {}, 10
    for d, m in ((64, 16), (512, 64)):
        rng = np.random.default_rng(d)
        N, nlist = 6000, 150
        X = rng.standard_normal((N, d)).astype(np.float32)
        X /= np.linalg.norm(X, axis=1, keepdims=True)
        ids = rng.permutation(10 * N)[:N].astype(np.int64)
        Q = X[rng.integers(0, N, 256)] + 0.05 * rng.standard_normal((256, d)).astype(np.float32)
        Qd = torch.from_numpy(Q).cuda()
        for name, idx in (("flat", IVFFlatIPIndex(d, nlist)), ("pq", IVFPQIPIndex(d, nlist, m))):
            tag = f"{name}{d}"
            idx.train(X)
            idx.add_with_ids(X[:4000], ids[:4000])
            idx.nprobe = 8
            arrays[f"{tag}.first.D"], arrays[f"{tag}.first.I"] = idx.search(Q[:3], k)
            idx.add_with_ids(torch.from_numpy(X[4000:]), torch.from_numpy(ids[4000:]))
            arrays[f"{tag}.centroids"] = idx.centroids.cpu().numpy()
            for i, a in enumerate(idx.lists_host()):
                arrays[f"{tag}.lists{i}"] = a
            for nprobe in (8, 128):
                idx.nprobe = nprobe
                for nq in (1, 256):
                    D, I = idx.search_device(Qd[:nq], k)
                    arrays[f"{tag}.p{nprobe}.q{nq}.D"], arrays[f"{tag}.p{nprobe}.q{nq}.I"] = D.cpu().numpy(), I.cpu().numpy()
                    if name == "flat":
                        cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
                        D, I = idx.search_local_device(Qd[:nq], k, probe_count=cnt)
                        arrays[f"{tag}.p{nprobe}.q{nq}.local.D"] = D.cpu().numpy()
                        arrays[f"{tag}.p{nprobe}.q{nq}.local.I"] = I.cpu().numpy()
                        arrays[f"{tag}.p{nprobe}.q{nq}.local.count"] = cnt.cpu().numpy()
            arrays[f"{tag}.reconstruct"] = idx.reconstruct_batch(np.concatenate([ids[[0, 17, 4500, N - 1]], [-5]]))
            arrays[f"{tag}.ntotal"] = np.array([idx.ntotal])
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    np.savez(out, **arrays)
    print(f"wrote {len(arrays)} arrays to {out}")


def compare(a, b) -> int:
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    for n in sorted(set(A.files) & set(B.files)):
        if A[n].dtype != B[n].dtype or A[n].shape != B[n].shape or A[n].tobytes() != B[n].tobytes():
            bad.append(n)
    print(f"{len(A.files)} arrays, {len(bad)} differ" + "".join(f"\n  {n}" for n in bad))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="ivf_identity.npz")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    sys.exit(compare(*args.compare) if args.compare else dump(args.out))

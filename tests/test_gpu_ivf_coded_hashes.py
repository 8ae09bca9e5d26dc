"""-m gpu: the whole surface of the inverted-file indexes whose lists hold encoded residuals (ivf_sq.py, ivf_pq.py), bit for bit.
tests/golden/ivf_coded_hashes.json holds SHA-256 digests of everything those classes hand back — state_host, encode_rows,
search_device with and without a selector, the rank-local searches of a slice adopted with pos_base, range_search_device,
reconstruct_batch — recorded on an MI355X from the commit the file names, BEFORE the classes moved onto CodedIVFIndexBase
(ivf_common.py).  One index per type, built once; one device.  The OPQ rotation is a signed permutation times one Givens
rotation with cosine 0.6 and sine 0.8, installed with set_rotation: no LAPACK result enters a digest.

Recording (on the GPU, from the commit to pin):  python tests/test_gpu_ivf_coded_hashes.py <commit> [<output.json>]"""
import functools
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

GOLDEN = Path(__file__).resolve().parent / "golden" / "ivf_coded_hashes.json"
N, D, NLIST, NPROBE, M, NQ, K = 4096, 32, 16, 4, 4, 5, 10
LO, HI = 1000, 3000                      # the slice a rank would hold
THRESH = 0.3
TYPES = ("IndexIVFSQ8", "IndexIVFSQfp16", "IVFPQ4", "IVFPQ4R8", "IVFPQ4R16", "IVFOPQ4", "IVFOPQ4R8")
ONE_PHASE = ("IndexIVFSQ8", "IndexIVFSQfp16", "IVFPQ4", "IVFOPQ4")


def _new(name):
    from wise_amd.index.ivf_pq import IVFOPQIPIndex, IVFOPQRefineIPIndex, IVFPQIPIndex, IVFPQRefineIPIndex
    from wise_amd.index.ivf_sq import IVFSQfp16IPIndex, IVFSQIPIndex
    idx = {"IndexIVFSQ8": lambda: IVFSQIPIndex(D, NLIST), "IndexIVFSQfp16": lambda: IVFSQfp16IPIndex(D, NLIST),
           "IVFPQ4": lambda: IVFPQIPIndex(D, NLIST, M), "IVFPQ4R8": lambda: IVFPQRefineIPIndex(D, NLIST, M, 8),
           "IVFPQ4R16": lambda: IVFPQRefineIPIndex(D, NLIST, M, 16), "IVFOPQ4": lambda: IVFOPQIPIndex(D, NLIST, M),
           "IVFOPQ4R8": lambda: IVFOPQRefineIPIndex(D, NLIST, M, 8)}[name]()
    idx.nprobe = NPROBE
    return idx


@functools.lru_cache(maxsize=None)
def _data():
    rng = np.random.default_rng(20)
    X = rng.standard_normal((N, D)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    ids = rng.permutation(3 * N)[:N].astype(np.int64)
    Q = X[:NQ] + np.float32(0.05) * rng.standard_normal((NQ, D)).astype(np.float32)
    return X, ids, np.ascontiguousarray(Q, dtype=np.float32)


def _rotation():
    """P G: a signed permutation of the axes times the Givens rotation (0.6, 0.8) of the first two — orthonormal in float32."""
    G = np.eye(D, dtype=np.float32)
    G[0, 0], G[0, 1], G[1, 0], G[1, 1] = 0.6, -0.8, 0.8, 0.6
    P = np.zeros((D, D), dtype=np.float32)
    for i in range(D):
        P[i, (7 * i + 3) % D] = -1.0 if i % 3 == 0 else 1.0
    return P @ G


@functools.lru_cache(maxsize=None)
def _index(name):
    X, ids, _ = _data()
    idx = _new(name)
    if "OPQ" in name:            # coarse quantizer and codebooks trained on the device, the rotation installed
        idx._coarse.train(X)
        idx.set_rotation(_rotation())
        xd = torch.from_numpy(X).to(idx.device)
        idx.set_codebooks(idx.train_codebooks(idx._rotate(idx.training_residuals(xd))))
    else:
        idx.train(X)
    idx.add_with_ids(X[:2500], ids[:2500], chunk=1000)
    idx.add_with_ids(X[2500:], ids[2500:], chunk=1000)
    return idx


def _slice(name, st):
    """A fresh index of the type that holds the rows [LO, HI) of the list-major arrays `st` (state_host of the whole index)."""
    loc = _new(name)
    loc.set_centroids(st["centroids"])
    if "trained" in st:
        loc.set_trained(st["trained"][:D], st["trained"][D:])
    if "codebooks" in st:
        loc.set_codebooks(st["codebooks"])
    if "rotation" in st:
        loc.set_rotation(st["rotation"])
    payload = st["halves"] if "halves" in st else st["codes"]
    extras = []
    if "rows" in st:
        rows = st["rows"][LO:HI]
        extras = [torch.from_numpy(rows if st["kind"] == 8 else rows.view(np.int16)),
                  None if st["scales"] is None else torch.from_numpy(st["scales"][LO:HI])]
    loc.adopt_lists(torch.from_numpy(payload[LO:HI]), torch.from_numpy(st["ids"][LO:HI]),
                    torch.from_numpy(np.clip(st["list_off"] - LO, 0, HI - LO)), *extras, pos_base=LO)
    assert loc.pos_base == LO and loc.ntotal == HI - LO
    return loc


def _digest(*values) -> str:
    h = hashlib.sha256()
    for v in values:
        if torch.is_tensor(v):
            v = v.cpu().numpy()
        if isinstance(v, np.ndarray):
            h.update(f"{v.dtype.str}{v.shape}".encode())
            h.update(np.ascontiguousarray(v).tobytes())
        else:
            h.update(repr(v).encode())
    return h.hexdigest()


def surface(name) -> dict:
    from wise_amd.index.selector import IDSelectorRange
    X, ids, Q = _data()
    idx = _index(name)
    q = torch.from_numpy(Q).to(idx.device)
    st = idx.state_host()
    out = {f"state_host.{key}": _digest(st[key]) for key in sorted(st)}
    out["encode_rows.300"] = _digest(*idx.encode_rows(X[:300], chunk=128))
    out["encode_rows.0"] = _digest(*idx.encode_rows(X[:0], chunk=128))
    out["search_device"] = _digest(*idx.search_device(q, K, chunk=2))
    out["search_device.sel"] = _digest(*idx.search_device(q, K, chunk=2, sel=IDSelectorRange(2000, 9000)))
    loc = _slice(name, st)
    if name in ONE_PHASE:
        out["search_local_device"] = _digest(*loc.search_local_device(q, K))
        count = torch.zeros(NQ, dtype=torch.int32, device=idx.device)
        out["search_local_device.probe_count"] = _digest(*loc.search_local_device(q, K, probe_count=count), count)
        out["search_local_device.positions"] = _digest(*loc.search_local_device(q, K, positions=True))
    else:
        cD, cand = loc.candidates_local_device(q, loc.candidates(K))
        out["candidates_local_device"] = _digest(cD, cand)
        out["refine_local_device"] = _digest(*loc.refine_local_device(q, cand, K))
    if "SQ" in name:
        out["range_search_device"] = _digest(*idx.range_search_device(q, THRESH))
    out["reconstruct_batch"] = _digest(idx.reconstruct_batch(np.concatenate([ids[100:109], [-5]]).astype(np.int64)))
    return out


def record(commit: str, path: Path = GOLDEN) -> None:
    """Write the golden file: run on the GPU from the commit whose behaviour is to be pinned."""
    path.write_text(json.dumps({"commit": commit, "hashes": {name: surface(name) for name in TYPES}}, indent=1) + "\n")


@pytest.mark.gpu
@pytest.mark.parametrize("name", TYPES)
def test_surface_equals_the_recorded_digests(name):
    want = json.loads(GOLDEN.read_text())["hashes"][name]
    got = surface(name)
    assert sorted(got) == sorted(want)
    assert got == want, sorted(key for key in want if got[key] != want[key])


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    record(sys.argv[1], Path(sys.argv[2]) if len(sys.argv) > 2 else GOLDEN)

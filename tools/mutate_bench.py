#!/usr/bin/env python
"""remove_ids beside the two ways of getting the same index without it, in one run -> profiles/mutate_bench.json.

Shape: --rows x --dim (default 10M x 512) clustered unit rows, IndexIVFFlat and IndexIVFSQ8, nlist = reference_nlist(rows).
Cases: 0.1 %, 10 % and 50 % of the ids removed, scattered (a seeded sample) and as one contiguous id range (ids are a seeded
permutation, so a range of ids is scattered over the lists too, but resolved by comparison instead of a binary search).
Per case, on the same device in the same process:
  remove   index.remove_ids(sel) on a copy of the lists (adopt_lists of cloned tensors; the clone is not timed)
  readd    a fresh index with the trained state set, add_with_ids of the kept rows from the host, lists merged
  rebuild  a fresh index, train on the seeded sample create_index draws, add_with_ids of the kept rows (once per type: it does
           not depend on the case beyond the row count; --no-rebuild skips it)
Reported: seconds (remove: median / min / max of --repeat runs; the others once — they take minutes), bytes/s on the kept rows'
bytes (payload + ids), peak extra device memory of remove_ids, and whether remove and readd left the same bytes.
Each timed section ends with a device synchronisation.  Nothing about the result is assumed beforehand."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from wise_amd.index.ivf_flat import IVFFlatIPIndex, reference_nlist      # noqa: E402
from wise_amd.index.ivf_sq import IVFSQIPIndex                           # noqa: E402
from wise_amd.index.selector import IDSelectorBatch, IDSelectorRange     # noqa: E402


def rows(n, d, centres, seed, chunk=1 << 18):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, d)).astype(np.float32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    out = np.empty((n, d), dtype=np.float32)
    for s in range(0, n, chunk):
        m = min(chunk, n - s)
        x = c[rng.integers(0, centres, m)] + np.float32(0.4 / np.sqrt(d)) * rng.standard_normal((m, d), dtype=np.float32)
        out[s:s + m] = x / np.linalg.norm(x, axis=1, keepdims=True)
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def new_index(kind, d, nlist, state=None):
    idx = IVFFlatIPIndex(d, nlist) if kind == "IndexIVFFlat" else IVFSQIPIndex(d, nlist)
    if state is not None:
        idx.set_centroids(state["centroids"])
        if kind == "IndexIVFSQ8":
            idx.set_trained(state["trained"][:d], state["trained"][d:])
    return idx


def add_all(idx, X, ids, step=1 << 20):
    for s in range(0, len(ids), step):
        idx.add_with_ids(X[s:s + step], ids[s:s + step])
    idx._finalize()
    return idx


def copy_of(kind, base, d, nlist, state):
    idx = new_index(kind, d, nlist, state)
    ls = base._lists
    idx.adopt_lists(ls.data.clone(), ls.ids.clone(), ls.list_off.clone())
    return idx


def state_bytes(idx):
    ls = idx._lists
    return [t.cpu().numpy() for t in (ls.data, ls.ids, ls.list_off)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-rebuild", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mutate_bench.json"))
    a = ap.parse_args()
    n, d = a.rows, a.dim
    nlist = reference_nlist(n)
    X = rows(n, d, max(nlist // 4, 8), 1)
    ids = np.random.default_rng(2).permutation(n).astype(np.int64)
    sample = np.sort(np.random.default_rng(1234).permutation(n)[:min(n, 100 * nlist)])
    result = {"rows": n, "dim": d, "nlist": nlist, "repeat": a.repeat, "device": torch.cuda.get_device_name(0), "cases": []}
    for kind in ("IndexIVFFlat", "IndexIVFSQ8"):
        base = new_index(kind, d, nlist)
        t_train, _ = timed(lambda: base.train(X[sample]))
        t_add, _ = timed(lambda: add_all(base, X, ids))
        state = {"centroids": base.centroids.cpu().numpy()}
        if kind == "IndexIVFSQ8":
            state["trained"] = base.trained.cpu().numpy()
        row_bytes = base._lists.data.shape[1] * base._lists.data.element_size() + 8
        for frac in (0.001, 0.1, 0.5):
            m = max(int(n * frac), 1)
            for shape in ("scattered", "range"):
                if shape == "scattered":
                    gone_ids = np.random.default_rng(7).permutation(ids)[:m]
                    sel, gone = IDSelectorBatch(gone_ids), np.isin(ids, gone_ids)
                else:
                    lo = n // 3
                    sel, gone = IDSelectorRange(lo, lo + m), (ids >= lo) & (ids < lo + m)
                times, peak, after = [], 0, None
                for _ in range(a.repeat):
                    idx = copy_of(kind, base, d, nlist, state)
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    before = torch.cuda.memory_allocated()
                    t, removed = timed(lambda: idx.remove_ids(sel))
                    peak = max(peak, torch.cuda.max_memory_allocated() - before)
                    assert removed == int(gone.sum())
                    times.append(t)
                    after = idx
                t_readd, re = timed(lambda: add_all(new_index(kind, d, nlist, state), X[~gone], ids[~gone]))
                same = all(np.array_equal(x, y) for x, y in zip(state_bytes(after), state_bytes(re)))
                kept_bytes = int((~gone).sum()) * row_bytes
                case = {"index": kind, "removed_fraction": frac, "shape": shape, "removed": int(gone.sum()),
                        "remove_s": {"median": float(np.median(times)), "min": min(times), "max": max(times)},
                        "remove_kept_bytes_per_s": kept_bytes / float(np.median(times)), "remove_peak_extra_bytes": int(peak),
                        "readd_s": t_readd, "same_bytes_as_readd": bool(same), "kept_bytes": kept_bytes}
                print(json.dumps(case), flush=True)
                result["cases"].append(case)
                del after, re
        result[kind + "_full_train_s"], result[kind + "_full_add_s"] = t_train, t_add
        if not a.no_rebuild:
            keep = ids % 2 == 1                                       # the 50 % case's row count
            fresh = new_index(kind, d, nlist)
            t, _ = timed(lambda: (fresh.train(X[keep][:min(int(keep.sum()), 100 * nlist)]), add_all(fresh, X[keep], ids[keep])))
            result[kind + "_rebuild_half_s"] = t
            del fresh
        del base
        torch.cuda.empty_cache()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

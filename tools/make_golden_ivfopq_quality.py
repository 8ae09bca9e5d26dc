"""Writes tests/golden/ivfopq_quality.json: what the float64 restatement of the OPQ trainer (tests/ivfopq_ref.py) reaches on the
seeded data of the CPU study.  CPU only, a few minutes:
    python tools/make_golden_ivfopq_quality.py

The data (ivfopq_ref.study_data / ivfopq_ref.STUDY): 20,000 x 64 unit rows around 64 unit centres; a row's offset from its centre
has per-coordinate deviation proportional to 1 / sqrt(1 + i), total length 0.6 in expectation, turned by a seeded random
orthogonal matrix (the "mixed spectrum"); rows re-normalised.  64 lists from ivfpq_ref.spherical_kmeans (seed 1234); m = 8; the
trainer at its defaults (first fit 10 Lloyd iterations, 50 outer iterations of 4).  200 queries = seeded rows nudged by 5 % noise;
recall@10 at nprobe 16 against the flat answer.

Recorded: the distortion after the fit of every outer iteration and the final one (training permutation seed 1234); the final
distortion and the recall for five seeds of the training permutation (its first 256 rows are the initial codewords);
distortion_margin = (max - min) / min of the five final distortions and recall_allowance = max - min of the five recalls — the
restatement's own spread, as in tests/golden/ivfpq_quality.json; and the recall of plain PQ (iteration 0's codebooks, R = I)."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import ivfopq_ref  # noqa: E402
import ivfpq_ref  # noqa: E402

SEEDS = [1234, 1, 2, 3, 4]


def main():
    p = ivfopq_ref.STUDY
    X, Q, c = ivfopq_ref.study_data()
    _, resid = ivfopq_ref.residuals(X, c)
    out = {"what": "ivfopq_ref.train (float64 restatement) on ivfopq_ref.study_data(): " + json.dumps(p), "seeds": SEEDS,
           "distortion": [], "recall_at_10": []}
    for seed in SEEDS:
        rt = resid[ivfpq_ref.training_rows(p["n"], seed)]
        R, cb, hist = ivfopq_ref.train(rt, p["m"])
        assert all(b <= a for a, b in zip(hist, hist[1:])), hist
        if seed == SEEDS[0]:
            out["distortion_per_iteration"] = hist
            cb_pq = ivfpq_ref.train(rt, p["m"], niter=10)
            out["distortion_pq"] = ivfpq_ref.distortion(rt, cb_pq)
            out["recall_at_10_pq"] = ivfopq_ref.recall_at_k(X, Q, c, None, cb_pq, p["nprobe"], p["k"])
        out["distortion"].append(hist[-1])
        out["recall_at_10"].append(ivfopq_ref.recall_at_k(X, Q, c, R, cb, p["nprobe"], p["k"]))
        print(seed, hist[0], hist[-1], out["recall_at_10"][-1], flush=True)
    dist = np.array(out["distortion"])
    out["distortion_margin"] = float((dist.max() - dist.min()) / dist.min())
    out["recall_allowance"] = float(max(out["recall_at_10"]) - min(out["recall_at_10"]))
    (ROOT / "tests" / "golden" / "ivfopq_quality.json").write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({k: v for k, v in out.items() if k != "distortion_per_iteration"}, indent=1))


if __name__ == "__main__":
    main()

"""tests/golden/ivf_l2_quality.json: recall@10 of IndexIVFFlatL2's method against the exact L2 answer on rows that are NOT normalised,
and beside it the recall of the spherical inner-product coarse quantizer (what the other inverted-file types train) over the same
rows — tests/ivf_l2_ref.recall_study for five seeds.  CPU only, numpy; no threshold is fixed in advance, the numbers are recorded.

    python tools/make_golden_ivf_l2_quality.py
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import ivf_l2_ref as ref  # noqa: E402


def main():
    seeds = [0, 1, 2, 3, 4]
    runs = []
    for s in seeds:
        runs.append(ref.recall_study(s))
        print(s, json.dumps(runs[-1]), flush=True)
    gold = {"what": "ivf_l2_ref.recall_study (numpy only, no GPU) for five seeds: " + json.dumps(ref.STUDY) + "; recall@10 against the "
                    "float64 exact L2 answer of IndexIVFFlatL2's method (plain k-means, probes by the largest x . c - |c|^2 / 2) and of "
                    "the spherical inner-product coarse quantizer over the same rows (exact L2 distances within its probed lists); "
                    "scanned_share = the mean share of the rows a query's probed lists hold; ip_top10_overlap_with_l2 = how much of "
                    "the exact L2 top 10 the exact inner-product top 10 holds (the rows' lengths spread over 4x)",
            "seeds": seeds, "runs": runs,
            "ivfflat_l2_min": min(r["ivfflat_l2"] for r in runs), "spherical_ip_coarse_min": min(r["spherical_ip_coarse"] for r in runs),
            "gap_min": min(r["ivfflat_l2"] - r["spherical_ip_coarse"] for r in runs),
            "gap_max": max(r["ivfflat_l2"] - r["spherical_ip_coarse"] for r in runs)}
    (ROOT / "tests" / "golden" / "ivf_l2_quality.json").write_text(json.dumps(gold, indent=1) + "\n")


if __name__ == "__main__":
    main()

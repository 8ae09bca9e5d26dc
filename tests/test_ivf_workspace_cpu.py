"""CPU test (-m "not gpu"): the scan workspace functions of the coded inverted-file indexes (IndexIVFSQ8 / IndexIVFSQfp16,
IndexIVFPQ<m>) answer what the library answered before the rank-local workspace layout moved into csrc/probe_compact.h.
tests/golden/ivf_workspace_bytes.json holds, per function, rows of [nq, nprobe, k(, m), bytes] recorded from that earlier
library over the full grid nq in {1, 2, 3, 255, 256, 511, 512, 513, 65535, 65536} x nprobe in {1, 2, 31, 32, 1024, 2048, 2049}
x k in {1, 10, 64, 65, 2048, 2049} (x m in {1, 4, 8, 64, 128, 129}), refused shapes (0 bytes) included.  The functions answer
without a device."""
import itertools
import json
from pathlib import Path

from wise_amd import _lib

GOLDEN = Path(__file__).resolve().parent / "golden" / "ivf_workspace_bytes.json"
NQ = (1, 2, 3, 255, 256, 511, 512, 513, 65535, 65536)
NPROBE = (1, 2, 31, 32, 1024, 2048, 2049)
K = (1, 10, 64, 65, 2048, 2049)
PQ_M = (1, 4, 8, 64, 128, 129)


def test_ivf_workspace_functions_return_the_recorded_bytes():
    lib = _lib.load()
    functions = json.loads(GOLDEN.read_text())["functions"]
    assert sorted(functions) == sorted(f"wise_{fam}_scan{part}_workspace_bytes" for fam in ("ivfsq", "ivfpq") for part in ("", "_local"))
    for name, rows in functions.items():
        fn = getattr(lib, name)
        grid = [list(a) for a in itertools.product(NQ, NPROBE, K, *((PQ_M,) if "ivfpq" in name else ()))]
        assert [r[:-1] for r in rows] == grid, name
        assert any(r[-1] == 0 for r in rows) and any(r[-1] > 0 for r in rows), name
        got = [[*r[:-1], int(fn(*r[:-1]))] for r in rows]
        assert got == rows, (name, [(g, r) for g, r in zip(got, rows) if g != r][:5])

"""The ledger of tests/test_gpu_gemm_tiles.py, without a GPU: every (variant, mode) kernel that tests/golden/gemm_plan.txt
says a tower launches, and every (variant, mode, producer) fold kernel, is in the case table the GPU module runs
(tests/gemm_tile_cases.py).  A tower shape that lands on a kernel with no direct test fails here.  The rest holds the
table to its own rules: what it calls refused the resolver's restatement refuses, what it runs the restatement accepts,
and the fold search still finds a shape for every fold row."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from tests import gemm_tile_cases as gc
from tests.gemm_tile_check import assert_epilogue as _assert_epilogue

ROOT = Path(__file__).resolve().parent.parent
LIB_DEBUG = ROOT / "wise_amd" / "lib" / "libwise_hip_debug.so"
GOLDEN = ROOT / "tests" / "golden" / "gemm_plan.txt"


def missing_from_table(text, plain_cases, fold_cases):
    """the kernels the plan table names and the case table lacks, each with one tower shape that launches it"""
    gemm, fold = gc.parse_plan_table(text)
    plain_cases, fold_cases = set(plain_cases), set(fold_cases)
    return ([f"gemm v={v} mode={m}: {line}" for (v, m), line in sorted(gemm.items()) if (v, m) not in plain_cases]
            + [f"fold v={v} mode={m} producer={p}: {line}" for (v, m, p), line in sorted(fold.items())
               if v != 0 and (v, m, p) not in fold_cases])


def test_every_kernel_the_towers_launch_has_a_direct_case():
    text = GOLDEN.read_text()
    gemm, fold = gc.parse_plan_table(text)
    assert len(gemm) >= 52 and len(fold) >= 30          # the parser sees the table (52 plain pairs when this was written)
    missing = missing_from_table(text, gc.PLAIN_CASES, gc.FOLD_CASES)
    assert not missing, "kernels with no case in tests/gemm_tile_cases.py:\n" + "\n".join(missing)


def test_the_ledger_notices_a_pair_that_leaves_the_table():
    text = GOLDEN.read_text()
    short = [c for c in gc.PLAIN_CASES if c != (68, gc.GELU)]
    assert [m.split(":")[0] for m in missing_from_table(text, short, gc.FOLD_CASES)] == ["gemm v=68 mode=2"]
    short = [c for c in gc.FOLD_CASES if c != (69, gc.F32, 1)]
    assert [m.split(":")[0] for m in missing_from_table(text, gc.PLAIN_CASES, short)] == ["fold v=69 mode=4 producer=1"]


def test_every_pair_is_run_or_listed_as_refused():
    assert set(gc.PLAIN_CASES) | set(gc.REFUSED) == {(v, m) for v in gc.VARIANTS for m in gc.MODES}
    assert not set(gc.PLAIN_CASES) & set(gc.REFUSED)
    assert set(gc.VARIANTS) == {0, 1, 2, 5, 40, 42, 44} | set(range(60, 71))


def _shapes(v):
    return [s[:3] for s in gc.persistent_shapes(256)] if v == gc.PERSISTENT else gc.plain_shapes(v)


def test_the_restated_resolver_runs_what_the_table_runs_and_refuses_what_it_refuses():
    for v, mode in gc.PLAIN_CASES:
        for M, N, K in _shapes(v):
            assert M % 128 == 0 and N % 4 == 0 and K % 32 == 0          # what gemm_bf16_rows takes
            assert gc.resolves(gc.FORCE_ID.get(v, v), M, N, K, mode) == v, (v, mode, M, N, K)
    for v, mode in gc.REFUSED:
        for M, N, K in _shapes(v):
            assert gc.resolves(v, M, N, K, mode) == 0, (v, mode, M, N, K)
    for v, K in gc.REFUSED_K:
        for tm, tn in gc.grids(v):
            assert gc.resolves(v, tm * gc.TILE[v][0], tn * gc.TILE[v][1], K, gc.F32) == 1


def _debug_lib():
    if not LIB_DEBUG.exists():
        pytest.skip("libwise_hip_debug.so not built (python -m wise_amd.build)")
    lib = C.CDLL(str(LIB_DEBUG))
    lib.wise_debug_gemm_plan.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.wise_debug_gemm_plan.restype = C.c_int
    return lib


def test_the_library_launches_what_the_table_says_under_every_force():
    """wise_debug_gemm_plan kind 3 (the plan under a forced id) on 256 CUs: one launch of the variant itself at every shape
    of the table, of variant 0 for the refused pairs, of variant 1 for the refused K — and the restatement says the same.
    Force id 0 is the plan's own choice, which is why variant 0 goes through FORCE_ID."""
    lib = _debug_lib()
    out = (C.c_int * 8)()

    def forced(force, M, N, K, mode):
        assert lib.wise_debug_gemm_plan(3, (C.c_int * 7)(force, M, N, K, mode, 256, 0), out) == 6
        return tuple(out[:3])

    for v in gc.VARIANTS:
        force = gc.FORCE_ID.get(v, v)
        assert force != 0
        for mode in gc.MODES:
            expect = v if (v, mode) in gc.PLAIN_CASES else 0
            for M, N, K in _shapes(v):
                assert forced(force, M, N, K, mode) == (0, 1, expect), (v, mode, M, N, K)
                assert gc.resolves(force, M, N, K, mode) == expect
    for v, K in gc.REFUSED_K:
        for tm, tn in gc.grids(v):
            assert forced(v, tm * gc.TILE[v][0], tn * gc.TILE[v][1], K, gc.F32) == (0, 1, 1)
    assert {forced(0, M, N, K, gc.BF16)[2] for M, N, K in gc.plain_shapes(0) if K == 1024 and N % 128 == 0} == {2}


def test_the_restated_resolver_keeps_every_variant_of_the_plan_table():
    """what gemm_plan answers went through resolve_variant already: the restatement must leave it as it is"""
    rows = 0
    for line in GOLDEN.read_text().splitlines():
        if not line.startswith("gemm"):
            continue
        left, right = line.split("->")
        M, N, K, mode = (int(re.search(rf"\b{k}=(\d+)", left).group(1)) for k in ("M", "N", "K", "mode"))
        parts = re.findall(r"\bv=(\d+)(?: x (\d+) rows)?", right)
        for v, r in parts:
            assert gc.resolves(int(v), int(r) if r else M, N, K, mode) == int(v), line
            rows += 1
    assert rows > 500


def test_tile_grids():
    for v in gc.VARIANTS:
        (a, b), rest = gc.grids(v)[0], gc.grids(v)[1:]
        assert b == (2 if v == 5 else 1) and a == {160: 4, 224: 4, 320: 2}.get(gc.TILE[v][0], 1)
        for tm, tn in rest:
            assert (tm * tn) % 8 != 0 and tm != tn and tn > 1 and (tm * gc.TILE[v][0]) % 128 == 0
            assert tm % 4 != 0 or gc.TILE[v][0] in (160, 224)
    assert {s[2] for s in gc.plain_shapes(60)} == {192, 256, 320, 1024}
    assert {s[2] for s in gc.plain_shapes(40)} == {96, 160, 192, 256, 320, 1024}
    assert {s[1] for s in gc.plain_shapes(1)} >= set(gc.N_EDGE)


@pytest.mark.parametrize("cus", [64, 104, 256, 304])
def test_persistent_tile_counts(cus):
    counts = []
    for M, N, K, modes in gc.persistent_shapes(cus):
        assert M % 640 == 0 and N % 256 == 0 and K in (512, 576) and set(modes) <= set(gc.BF16_MODES)
        counts.append((M // 160) * (N // 256))
    small, one, two = sorted(set(counts))
    assert small == 12 < cus and cus < one <= cus + 4 and 2 * cus < two <= 2 * cus + 4
    if cus == 256:
        assert (one, two) == (260, 516)


def test_the_fold_search_finds_a_shape_for_every_fold_row():
    lib = _debug_lib()
    out = (C.c_int * 8)()

    def plan(*a):
        assert lib.wise_debug_gemm_plan(1, (C.c_int * 7)(*a), out) == 1
        return out[0]

    for v, mode, producer in gc.FOLD_CASES:
        found = [s for wide96 in ((0, 1) if producer else (0,)) for s in gc.fold_shapes(plan, 256, v, mode, producer, wide96)]
        assert found, (v, mode, producer)
        for M, N, K in found:
            assert M * N * K <= 8e9, (v, mode, producer, M, N, K)      # a reference the CPU makes in about a second
    # the 96-column tiles keep statistics per 32 columns only: no producer there without group32
    assert gc.fold_shapes(plan, 256, 67, gc.RESID, 1, 0) == []


def test_the_gpu_modules_checker_notices_what_a_wrong_kernel_would_give():
    """_assert_epilogue of tests/test_gpu_gemm_tiles.py on made-up outputs, on the CPU: the exact output passes; one bf16
    value next to the right one, two swapped 16-column fragments, a displaced row, one fp32 last bit, an activation 2^-7
    off and a NaN do not."""
    g = torch.Generator().manual_seed(5)
    pre = torch.randint(-2048, 2049, (64, 128), generator=g).float() / 16
    resid = torch.randint(-1024, 1025, (64, 128), generator=g).float() / 16

    def right(mode):
        if mode in (gc.RESID, gc.F32):
            return pre + resid if mode == gc.RESID else pre.clone()
        if mode in (gc.BF16, gc.RELU):
            return (pre.clamp(min=0) if mode == gc.RELU else pre).to(torch.bfloat16)
        x = pre.double()
        want = {gc.QUICKGELU: x * torch.sigmoid(1.702 * x), gc.GELU: 0.5 * x * (1 + torch.erf(x / 2 ** 0.5)),
                gc.GELU_TANH: 0.5 * x * (1 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))}[mode]
        return want.to(torch.bfloat16)

    def swapped(t):
        t = t.clone()
        t[:16, :16], t[:16, 16:32] = t[:16, 16:32].clone(), t[:16, :16].clone()
        return t

    def next_value(t):
        t = t.clone()
        bits = t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
        bits[63, 127] += 1
        return t

    def scaled(t):
        return (t.double() * (1 + 2.0 ** -7)).to(t.dtype)

    def with_nan(t):
        t = t.clone()
        t[5, 7] = float("nan")
        return t

    for mode in gc.MODES:
        good = right(mode)
        _assert_epilogue(good, pre, mode, "exact", resid)
        exact = mode in (gc.BF16, gc.RELU, gc.RESID, gc.F32)
        for wrong in (swapped, lambda t: torch.roll(t, 1, 0), with_nan, scaled) + ((next_value,) if exact else ()):
            bad = wrong(good)
            assert not torch.equal(bad.float(), good.float()) or wrong is with_nan
            with pytest.raises(AssertionError):
                _assert_epilogue(bad, pre, mode, "wrong", resid)

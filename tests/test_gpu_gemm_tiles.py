"""-m gpu: every tile form and epilogue of the bf16 GEMM family (csrc/gemm_bf16.hip, csrc/gemm_w4.h), kernel by kernel.

The planner picks a tile by shape, so a tower reaches most (tile, epilogue) kernels at a few batch sizes only, and the tower
tests see them through a cosine over 12 or 24 layers.  Here every pair of tests/gemm_tile_cases.py is launched directly:
the plain GEMM with the variant forced through the debug library (wise_debug_set_gemm_variant + wise_debug_gemm_rows), the
two LayerNorm-fold forms at shapes fold_plan itself sends to each tile (asserted through wise_debug_gemm_plan).  The shapes
are a few tiles: grids whose tile count is no multiple of 8 and whose rows are no multiple of the group, 3 / 4 / 5 / 16
K-steps, and for the persistent form one, two and three tiles per workgroup.

Exact data.  A: integers in [-2, 2]; W: integers in [-2, 2] / 16; bias: multiples of 1/16, |b| <= 4; residual: multiples of
1/16, |x| <= 64; rstd (fold consumer): 1/2, 1/4, 1/8.  With K <= 4096 every partial sum is a multiple of 2^-4 below 2^11
(2^-7 and 18 bits with the row scale): exact in fp32 in ANY order of accumulation.  So the reference is one fp32 matmul on
the CPU (test_references_agree holds it to float64), and
  modes 3, 4            torch.equal(got, ref)
  mode 0, mode 6        torch.equal(got, bf16(ref)), torch.equal(got, bf16(relu(ref)))      (round to nearest even)
  modes 1, 2, 5         |got - want| <= 2^-8 |want| + 5e-5 against the float64 activation of the exact pre-activation:
                        one bf16 rounding is 2^-9 relative, the erf-GELU fit is within 2.6e-5 (gemm_shared.h), the other
                        two are one exp2 and one rcp — a factor two over each term, nothing measured.
Every output sits between 128 guard rows in front and behind, which must come back untouched."""
import ctypes as C
import functools

import pytest
import torch

from tests import gemm_tile_cases as gc
from tests.gemm_tile_check import assert_epilogue as _assert_epilogue, where as _where
from wise_amd import _lib

pytestmark = pytest.mark.gpu

_P = C.c_void_p
GUARD_ROWS = 128
BF16_GUARD = 0x7FC1             # a NaN no kernel produces
F32_GUARD = 0x7FC12345          # the same in fp32
RESID_GUARD = 12345.0           # mode 3 reads its output: finite sentinels
EPS = 1e-5


@functools.lru_cache(maxsize=None)
def _dbg():
    d = _lib.load_debug()
    d.wise_debug_set_gemm_variant.argtypes = [C.c_int]
    d.wise_debug_set_gemm_variant.restype = C.c_int
    d.wise_debug_gemm_plan.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    d.wise_debug_gemm_plan.restype = C.c_int
    d.wise_debug_gemm_rows.argtypes = [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]
    d.wise_debug_gemm_rows.restype = C.c_int
    return d


@functools.lru_cache(maxsize=None)
def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


@pytest.fixture(autouse=True)
def _plans_own_choice_afterwards():
    """whatever a case forced, the next test (of any module that loads the debug library) gets the plan's own choice"""
    yield
    _dbg().wise_debug_set_gemm_variant(0)


# ---------------------------------------------------------------------------------------------------------------------
# data and references
# ---------------------------------------------------------------------------------------------------------------------
def _operands(M, N, K):
    """A, W (fp32 on the CPU, exact in bf16) and the bias of one shape: seeded random values, so W has no symmetry that
    could hide a transposed or displaced fragment"""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
    A = torch.randint(-2, 3, (M, K), generator=g, dtype=torch.int8).float()
    W = torch.randint(-2, 3, (N, K), generator=g, dtype=torch.int8).float() / 16
    bias = torch.randint(-64, 65, (N,), generator=g).float() / 16
    return A, W, bias


@functools.lru_cache(maxsize=24)
def _problem(M, N, K):
    """Operands of one shape on the device and the exact product A @ W^T (fp32 matmul on the CPU, made once per shape and
    shared by every mode; nobody writes to it)."""
    A, W, bias = _operands(M, N, K)
    return {"A": A.to(torch.bfloat16).cuda(), "W": W.to(torch.bfloat16).cuda(), "bias": bias.cuda(), "prod": (A @ W.t()).cuda()}


@functools.lru_cache(maxsize=8)
def _resid(M, N):
    g = torch.Generator().manual_seed(7919 * M + N)
    return (torch.randint(-1024, 1025, (M, N), generator=g, dtype=torch.int16).float() / 16).cuda()


def test_references_agree():
    """the fp32 matmul the module uses as reference is the float64 one, bit for bit (the data's point), and far from trivial"""
    M, N, K = 384, 288, 1024
    A, W, _ = _operands(M, N, K)
    ref32 = A @ W.t()
    assert torch.equal(ref32.double(), A.double() @ W.double().t())
    assert torch.equal(ref32, _problem(M, N, K)["prod"].cpu())
    assert torch.equal(ref32 * 16, (ref32 * 16).round()) and 3.0 < ref32.std().item() < 5.0 and ref32.abs().max().item() < 2048
    assert not torch.equal(W[:N, :N], W[:N, :N].t())


class _Guarded:
    """[rows, N] of `dtype` between GUARD_ROWS guard rows in front and behind, all of it filled with one bit pattern"""

    def __init__(self, rows, N, mode):
        f32 = mode in (gc.RESID, gc.F32)
        self.full = torch.empty(rows + 2 * GUARD_ROWS, N, dtype=torch.float32 if f32 else torch.bfloat16, device="cuda")
        self.bits = self.full.view(torch.int32 if f32 else torch.int16)
        if mode == gc.RESID:
            self.full.fill_(RESID_GUARD)
        else:
            self.bits.fill_(F32_GUARD if f32 else BF16_GUARD)
        self.pattern = int(self.bits[0, 0])
        self.body = self.full[GUARD_ROWS:GUARD_ROWS + rows]

    def intact(self):
        g = GUARD_ROWS
        return bool((self.bits[:g] == self.pattern).all()) and bool((self.bits[-g:] == self.pattern).all())


# ---------------------------------------------------------------------------------------------------------------------
# plain GEMM, the variant forced
# ---------------------------------------------------------------------------------------------------------------------
def _forced_plan(force, M, N, K, mode):
    """what gemm_bf16_rows launches on this device under wise_debug_set_gemm_variant(force): (splitk, launches, variant)"""
    out = (C.c_int * 8)()
    assert _dbg().wise_debug_gemm_plan(3, (C.c_int * 7)(force, M, N, K, mode, _cus(), 0), out) == 6
    return out[0], out[1], out[2]


def _forced(v, mode, M, N, K, with_bias, expect=None):
    """One launch with variant v forced; checks it against the exact reference.  expect: the variant that runs (v itself;
    the fallback of a refused pair).  resolve_variant falls back to 0 or 1 without a word, and force id 0 means "the plan's
    own choice" (variant 0 is forced through gc.FORCE_ID): so the library's own plan under this force, on this device, must
    name ONE launch of the expected variant before anything is launched — and the restatement of the case table agree."""
    expect = v if expect is None else expect
    force = gc.FORCE_ID.get(v, v)
    rows, cols = gc.TILE[expect]
    what = f"v={v}{'' if expect == v else f' (runs {expect})'} mode={mode} M={M} N={N} K={K} " \
           f"({M // rows} x {-(-N // cols)} tiles, {K / 64:g} K-steps of 64){'' if with_bias else ' no bias'}"
    assert force != 0 and _forced_plan(force, M, N, K, mode) == (0, 1, expect), what
    assert gc.resolves(force, M, N, K, mode) == expect, what
    p = _problem(M, N, K)
    out = _Guarded(M, N, mode)
    resid = None
    if mode == gc.RESID:
        resid = _resid(M, N)
        out.body.copy_(resid)
    d = _dbg()
    assert d.wise_debug_set_gemm_variant(force) == 0
    rc = d.wise_debug_gemm_rows(p["A"].data_ptr(), p["W"].data_ptr(), p["bias"].data_ptr() if with_bias else None, M, 0, N, K,
                                mode, out.body.data_ptr(), None, 0, _lib.stream_ptr())
    assert rc == 0, f"{what}: {d.wise_last_error().decode()}"
    torch.cuda.synchronize()
    assert out.intact(), f"{what}: guard rows written"
    _assert_epilogue(out.body, p["prod"] + p["bias"] if with_bias else p["prod"], mode, what, resid)


@pytest.mark.parametrize("v,mode", [pytest.param(v, m, id=f"v{v}-mode{m}") for v, m in gc.PLAIN_CASES if v != gc.PERSISTENT])
def test_forced_tile(v, mode):
    """every grid x every K-step count of the variant (and the N edge of variants 0 and 1); every fifth shape without a bias"""
    shapes = gc.plain_shapes(v)
    assert len(shapes) >= 6
    for i, (M, N, K) in enumerate(shapes):
        _forced(v, mode, M, N, K, with_bias=i % 5 != 1)


@pytest.mark.parametrize("K", [512, 576])
@pytest.mark.parametrize("walk", ["one_tile", "two_tiles", "three_tiles"])
def test_forced_persistent_tile(walk, K):
    """Variant 64, the persistent 160 x 256 form, on the device's own CU count: fewer tiles than CUs; some workgroups with two
    tiles and the rest with one; some with three (the t > 0 path twice in a workgroup) — at 8 and 9 K-steps."""
    cus = _cus()
    shapes = [s for s in gc.persistent_shapes(cus) if s[2] == K]
    M, N, _, modes = shapes[("one_tile", "two_tiles", "three_tiles").index(walk)]
    tiles = (M // 160) * (N // 256)
    assert {"one_tile": tiles < cus, "two_tiles": cus < tiles <= 2 * cus, "three_tiles": 2 * cus < tiles <= 3 * cus}[walk]
    for i, mode in enumerate(modes):
        _forced(gc.PERSISTENT, mode, M, N, K, with_bias=not (walk == "one_tile" and i == 1))


def test_refused_pairs_fall_back():
    """What the case table lists as refused the library runs on variant 0 / 1, as its plan says, and still gets right: the
    fp32 modes on the bf16-only tiles, K % 64 != 0 on the 320 x 128 ping-pong tile."""
    for v, mode in gc.REFUSED:
        _forced(v, mode, 640, gc.TILE[v][1] * 2, 512, True, expect=0)
    for v, K in gc.REFUSED_K:
        _forced(v, gc.F32, 640, 256, K, True, expect=1)


def test_force_id_zero_is_the_plans_own_choice():
    """why variant 0 is forced through gc.FORCE_ID: under force 0 the 16-step shapes of variant 0 run the 64-deep ring"""
    assert gc.FORCE_ID[0] != 0
    M, N, K = next(x for x in gc.plain_shapes(0) if x[2] == 1024 and x[1] % 128 == 0)
    assert _forced_plan(0, M, N, K, gc.BF16)[2] == 2 and _forced_plan(gc.FORCE_ID[0], M, N, K, gc.BF16) == (0, 1, 0)


# ---------------------------------------------------------------------------------------------------------------------
# fold forms: shapes through fold_plan
# ---------------------------------------------------------------------------------------------------------------------
def _fold_plan(M, N, K, mode, producer, wide96, cus):
    out = (C.c_int * 8)()
    assert _dbg().wise_debug_gemm_plan(1, (C.c_int * 7)(M, N, K, mode, producer, wide96, cus), out) == 1
    return out[0]


@functools.lru_cache(maxsize=None)
def _fold_shapes(v, mode, producer, wide96):
    return tuple(gc.fold_shapes(_fold_plan, _cus(), v, mode, producer, wide96))


def _consumer(v, mode, M, N, K):
    what = f"fold consumer v={v} mode={mode} M={M} N={N} K={K}"
    assert gc.fold_shape_ok(M, N, K, 0, 0) and _fold_plan(M, N, K, mode, 0, 0, _cus()) == v, what
    p = _problem(M, N, K)
    i = torch.arange(M, device="cuda")
    rstd = 2.0 ** -(1 + (i * 5 + i // 7) % 3).float()             # 1/2, 1/4, 1/8, in no tile's period
    out = _Guarded(M, N, mode)
    lib = _lib.lib()
    _lib.check(lib.wise_gemm_fold_bf16(p["A"].data_ptr(), p["W"].data_ptr(), p["bias"].data_ptr(), rstd.data_ptr(), M, N, K, mode,
                                       out.body.data_ptr(), _lib.stream_ptr()), "wise_gemm_fold_bf16")
    torch.cuda.synchronize()
    assert out.intact(), f"{what}: guard rows written"
    _assert_epilogue(out.body, rstd[:, None] * p["prod"] + p["bias"], mode, what)


def _bits(t):
    return t.view(torch.int16)


class _Stream:
    """A residual stream x = hi + lo as wise_gemm_fold_resid takes it (two [M, N] bf16 arrays, lo behind hi), with guard rows
    in front, between and behind, and the statistics scratch between guards of its own."""

    def __init__(self, M, N):
        g = GUARD_ROWS
        self.M, self.N = M, N
        self.full = torch.full((2 * M + 3 * g, N), BF16_GUARD, dtype=torch.int16, device="cuda")
        self.hi = self.full[g:g + M].view(torch.bfloat16)
        self.lo = self.full[2 * g + M:2 * g + 2 * M].view(torch.bfloat16)
        self.lo_off = (g + M) * N
        lib = _lib.lib()
        words = lib.wise_gemm_fold_stats_bytes(M, N) // 4
        assert words >= M + M * (N // 32) * 2 + M // 128 + 1
        self.sfull = torch.full((words + 512,), F32_GUARD, dtype=torch.int32, device="cuda")     # NaN wherever nothing is written
        self.stats = self.sfull[256:256 + words].view(torch.float32)
        o, n = lib.wise_gemm_fold_counters_offset(M) // 4, lib.wise_gemm_fold_counters_bytes(M) // 4
        self.counters = self.sfull[256 + o:256 + o + n]
        self.counters.zero_()                                     # only the counters must be zero on entry

    def intact(self):
        g, M = GUARD_ROWS, self.M
        return all(bool((t == BF16_GUARD).all()) for t in (self.full[:g], self.full[g + M:2 * g + M], self.full[-g:])) and \
            bool((self.sfull[:256] == F32_GUARD).all()) and bool((self.sfull[-256:] == F32_GUARD).all())

    def launch(self, p, K, group32, start, with_bias=True):
        lib = _lib.lib()
        _lib.check(lib.wise_gemm_fold_resid(p["A"].data_ptr(), p["W"].data_ptr(), p["bias"].data_ptr() if with_bias else None, self.M, self.N, K,
                                            self.hi.data_ptr(), self.lo_off, self.stats.data_ptr(), EPS, group32 | (2 if start else 0),
                                            _lib.stream_ptr()), "wise_gemm_fold_resid")
        torch.cuda.synchronize()


def _producer(v, start, group32, M, N, K, with_bias=True):
    mode = gc.F32 if start else gc.RESID
    what = f"fold producer v={v} {'start' if start else 'accumulate'} group32={group32} M={M} N={N} K={K}{'' if with_bias else ' no bias'}"
    assert gc.fold_shape_ok(M, N, K, 1, group32) and _fold_plan(M, N, K, mode, 1, group32, _cus()) == v, what
    p = _problem(M, N, K)
    row = p["prod"] + p["bias"] if with_bias else p["prod"]
    s = _Stream(M, N)
    if start:
        before = None                       # hi and lo hold the NaN pattern: the form that starts a stream must not read them
    else:
        x0 = _resid(M, N)
        before = (x0.to(torch.bfloat16), (x0 - x0.to(torch.bfloat16).float()).to(torch.bfloat16))
        assert torch.equal(before[0].float() + before[1].float(), x0)
        s.hi.copy_(before[0])
        s.lo.copy_(before[1])
        row = row + x0
    s.launch(p, K, group32, start, with_bias)
    assert s.intact(), f"{what}: guard rows written"
    hi, lo = s.hi.clone(), s.lo.clone()
    # at most 15 significant bits in a row's values: hi + lo carries them all
    assert torch.equal(hi.float() + lo.float(), row), _where(hi.float() + lo.float() != row, what + " hi + lo")
    assert torch.equal(hi, row.to(torch.bfloat16)), _where(hi != row.to(torch.bfloat16), what + " hi")
    assert torch.equal(lo, (row - hi.float()).to(torch.bfloat16)), what + " lo"
    rstd = s.stats[:M].double()
    want = 1.0 / torch.sqrt(row.double().var(dim=1, unbiased=False) + EPS)
    rel = ((rstd - want).abs() / want).max().item()
    print(f"{what}: rstd max relative error {rel:.2e}")
    assert rel <= 2e-5, f"{what}: rstd {rel}"                   # (a NaN fails)
    assert int(s.counters.abs().max()) == 0, f"{what}: counters left non-zero"
    # the same launch on the same scratch (for the starting form: over other NaNs): the same bits
    rstd_bits = s.stats[:M].clone().view(torch.int32)
    if start:
        _bits(s.hi).fill_(-1)
        _bits(s.lo).fill_(-1)
    else:
        s.hi.copy_(before[0])
        s.lo.copy_(before[1])
    s.launch(p, K, group32, start, with_bias)
    assert s.intact()
    assert torch.equal(_bits(s.hi), _bits(hi)) and torch.equal(_bits(s.lo), _bits(lo)), what + " second launch"
    assert torch.equal(s.stats[:M].view(torch.int32), rstd_bits) and int(s.counters.abs().max()) == 0, what + " second launch"


@pytest.mark.parametrize("v,mode,producer", [pytest.param(*c, id=f"v{c[0]}-mode{c[1]}-{'producer' if c[2] else 'consumer'}")
                                             for c in gc.FOLD_CASES])
def test_fold_tile(v, mode, producer):
    """The smallest shape fold_plan sends to the tile on this device, at 3, 4 and 5 K-steps where it stays there.  Producers
    (mode 3: x += ..., mode 4: the rows that start a stream) with statistics per 64 and per 32 columns, whichever the
    plan gives this tile for."""
    ran = 0
    for group32 in ((0, 1) if producer else (0,)):
        shapes = _fold_shapes(v, mode, producer, group32)
        for i, (M, N, K) in enumerate(shapes):
            if producer:      # (the producer takes a null bias, the consumer does not: the last of several shapes goes without)
                _producer(v, mode == gc.F32, group32, M, N, K, with_bias=len(shapes) == 1 or i + 1 < len(shapes))
            else:
                _consumer(v, mode, M, N, K)
            ran += 1
    assert ran, f"fold_plan sends no searched shape to variant {v} (mode {mode}, producer {producer}) on {_cus()} CUs"

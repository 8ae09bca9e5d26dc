"""-m gpu: the skinny GEMM path of the text towers (csrc/gemm_bf16.hip: gemm_bf16_rows / gemm_resid_ln_rows), kernel by kernel.

A call with at most 128 rows of data splits K: gemm_splitk_kernel<4> writes S fp32 partial tiles into the caller's scratch,
then splitk_reduce_kernel<MODE> (bias + epilogue) or splitk_reduce_ln_kernel<NV> (bias + residual + LayerNorm) adds them.
None of the three has a C entry of its own, so the debug library exports the two host functions as the towers call them
(wise_debug_gemm_rows, wise_debug_gemm_resid_ln_rows) and the scratch size (wise_debug_gemm_splitk_bytes).

Every reference is float64 torch on the CPU from the bf16-rounded inputs, inputs scaled as in test_gpu_vit.test_gemm_modes
(A ~ N(0,1), W ~ N(0,1) K^-0.5, bias ~ N(0,1)), and every case first asks the plan how many slices it takes, so that a
case cannot pass by taking another path than the one it names.

Bounds (none is fitted to what the kernels give):
  fp32 outputs (modes 3, 4)            |got - ref| <= 2e-3                     test_gemm_modes' bound at this input scale
  bf16 outputs (modes 0, 1, 2, 5, 6)   |got - ref| <= 2^-8 |ref| + 1.13 * 2e-3   one bf16 rounding + the fp32 bound through an
                                                                             activation (1.13: the largest slope of GELU / QuickGELU)
  LayerNorm h                          |h - bf16(h_ref)| <= 2^-7 max|h_ref|      test_layernorm's bound
  post-LN x                            |x - h_ref| <= 2e-3 max|ln_w| rstd_max + 1e-5
"""
import ctypes as C
import functools

import pytest
import torch

from wise_amd import _lib

pytestmark = pytest.mark.gpu

_P = C.c_void_p
BF16, QUICKGELU, GELU, RESID, F32, GELU_TANH, RELU = 0, 1, 2, 3, 4, 5, 6
MODES = (BF16, QUICKGELU, GELU, RESID, F32, GELU_TANH, RELU)
CUS = 256
F32_TOL = 2e-3
ACT_SLOPE = 1.13
EPS = 1e-5
GUARD = 4096

# K -> (slices S, 64-deep K-tiles per slice; the ring has 4 stages, 3 of them staged by the prologue), by hand from
# splitk_slices for N in {128, 384}; test_plan_splits_as_the_table_says holds the plan to it
K_TABLE = {640: (2, 5), 512: (4, 2), 768: (4, 3), 1792: (4, 7), 1024: (8, 2), 2048: (16, 2), 4096: (32, 2)}
M_VALID = (1, 77, 128)


@functools.lru_cache(maxsize=None)
def _dbg():
    d = _lib.load_debug()
    d.wise_debug_gemm_plan.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    d.wise_debug_gemm_plan.restype = C.c_int
    d.wise_debug_gemm_splitk_bytes.argtypes = [C.c_int] * 4
    d.wise_debug_gemm_splitk_bytes.restype = C.c_size_t
    d.wise_debug_gemm_rows.argtypes = [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]
    d.wise_debug_gemm_rows.restype = C.c_int
    d.wise_debug_gemm_resid_ln_rows.argtypes = [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_float,
                                                C.c_int, _P, _P, C.c_size_t, _P]
    d.wise_debug_gemm_resid_ln_rows.restype = C.c_int
    return d


def _ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"debug library {what} failed (rc={rc}): {_dbg().wise_last_error().decode()}")


def _plan_splitk(M, N, K, mode, m_valid):
    a = (C.c_int * 7)(M, N, K, mode, m_valid, 0, CUS)
    out = (C.c_int * 8)()
    assert _dbg().wise_debug_gemm_plan(0, a, out) == 6
    return out[0]


def _need(M, m_valid, N, K):
    return int(_dbg().wise_debug_gemm_splitk_bytes(M, m_valid, N, K))


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


@functools.lru_cache(maxsize=None)
def _problem(M, N, K):
    """Seeded inputs of one shape, their device copies and the float64 product — made once, shared, never written to."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
    A = bf16_round(torch.randn(M, K, generator=g))
    W = bf16_round(torch.randn(N, K, generator=g) * K ** -0.5)
    bias = torch.randn(N, generator=g)
    resid = torch.randn(M, N, generator=g)
    return {"A": A.to(torch.bfloat16).cuda(), "W": W.to(torch.bfloat16).cuda(), "bias": bias.cuda(), "resid": resid,
            "prod": A.double() @ W.double().t(), "bias64": bias.double()}


def _epilogue_ref(pre, mode, resid):
    if mode == RESID:
        return pre + resid.double()
    if mode == QUICKGELU:
        return pre * torch.sigmoid(1.702 * pre)
    if mode == GELU:
        return 0.5 * pre * (1 + torch.erf(pre / 2 ** 0.5))
    if mode == GELU_TANH:
        return 0.5 * pre * (1 + torch.tanh(0.7978845608028654 * (pre + 0.044715 * pre ** 3)))
    if mode == RELU:
        return pre.clamp(min=0)
    return pre


def _guarded(nbytes, dtype, fill=None):
    """A device buffer of nbytes with a 4 KiB canary behind it: (the typed view of the buffer, the canary's view)."""
    raw = torch.empty(nbytes + GUARD, dtype=torch.uint8, device="cuda")
    raw[nbytes:] = 0xA5
    buf = raw[:nbytes].view(dtype)
    if fill is not None:
        buf.fill_(fill)
    return buf, raw[nbytes:]


def _intact(canary):
    return bool((canary == 0xA5).all().item())


def _out_for(p, M, N, mode):
    """The output buffer of one call (the residual stream for mode 3) with its canary."""
    if mode == RESID:
        out, can = _guarded(M * N * 4, torch.float32)
        out.view(M, N).copy_(p["resid"])
    elif mode == F32:
        out, can = _guarded(M * N * 4, torch.float32, float("nan"))
    else:
        out, can = _guarded(M * N * 2, torch.bfloat16, float("nan"))
    return out.view(M, N), can


def _run_rows(p, M, m_valid, N, K, mode, with_bias, sk, sk_bytes, A=None):
    out, can = _out_for(p, M, N, mode)
    Ad = p["A"] if A is None else A
    _ok(_dbg().wise_debug_gemm_rows(Ad.data_ptr(), p["W"].data_ptr(), p["bias"].data_ptr() if with_bias else None, M, m_valid,
                                    N, K, mode, out.data_ptr(), None if sk is None else sk.data_ptr(), sk_bytes,
                                    _lib.stream_ptr()), "gemm_rows")
    torch.cuda.synchronize()
    return out, can


def _assert_rows(out, p, m_valid, mode, with_bias):
    pre = p["prod"][:m_valid] + (p["bias64"] if with_bias else 0.0)
    ref = _epilogue_ref(pre, mode, p["resid"][:m_valid])
    got = out[:m_valid].float().cpu().double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    if mode in (RESID, F32):
        print(f"max |got - ref| = {err.max().item():.3e} (bound {F32_TOL:.1e})")
        assert err.max().item() <= F32_TOL
    else:
        tol = 2.0 ** -8 * ref.abs() + ACT_SLOPE * F32_TOL
        print(f"max |got - ref| / bound = {(err / tol).max().item():.3f}, max |got - ref| = {err.max().item():.3e}")
        assert (err <= tol).all(), (err - tol).max().item()


def _rows_M(mode):
    # mode 6 reached the fp32 reduction before it had a case of its own: its out has 256 rows, so that even that write
    # (m_valid * N * 4 bytes <= 128 * N * 4 = 256 * N * 2) would have stayed inside the allocation
    return 256 if mode == RELU else 128


# ---------------------------------------------------------------- a. every slice count, every ring depth, against float64
def _split_cases():
    """every K row x every mode, three cases each: every m_valid once, N and the bias alternating from case to case"""
    out = []
    for ki, K in enumerate(K_TABLE):
        for mi, mode in enumerate(MODES):
            i = ki * len(MODES) + mi
            for j, mv in enumerate(M_VALID):
                N = (128, 384)[(i + j) % 2]
                with_bias = ((i + j) // 2) % 2 == 0
                out.append(pytest.param(K, N, mv, mode, with_bias, id=f"K{K}-N{N}-mv{mv}-mode{mode}-{'bias' if with_bias else 'nobias'}"))
    return out


def test_plan_splits_as_the_table_says():
    seen_s, seen_tiles = set(), set()
    for K, (S, tiles) in K_TABLE.items():
        for N in (128, 384):
            for mode in MODES:
                for mv in M_VALID:
                    M = _rows_M(mode)
                    assert _plan_splitk(M, N, K, mode, mv) == S, (K, N, mode, mv)
                    assert _need(M, mv, N, K) == S * 128 * N * 4
        assert K % (S * 64) == 0 and K // S // 64 == tiles
        seen_s.add(S)
        seen_tiles.add(tiles)
    assert seen_s == {2, 4, 8, 16, 32} and seen_tiles == {2, 3, 5, 7}


@pytest.mark.parametrize("K,N,m_valid,mode,with_bias", _split_cases())
def test_splitk_against_float64(K, N, m_valid, mode, with_bias):
    """gemm_splitk_kernel<4> + splitk_reduce_kernel<mode> on rows < m_valid.  Mode 6 (ReLU, bf16): the reduction used to
    have no case for it and wrote fp32 sums into the bf16 output."""
    M = _rows_M(mode)
    S = K_TABLE[K][0]
    assert _plan_splitk(M, N, K, mode, m_valid) == S
    need = _need(M, m_valid, N, K)
    assert need == S * 128 * N * 4
    p = _problem(M, N, K)
    sk, sk_can = _guarded(need, torch.float32, float("nan"))
    out, out_can = _run_rows(p, M, m_valid, N, K, mode, with_bias, sk, need)
    assert _intact(out_can) and _intact(sk_can)
    assert not torch.isnan(sk).any()      # all S partial tiles were written: the split path ran, and with S slices
    _assert_rows(out, p, m_valid, mode, with_bias)


# ---------------------------------------------------------------- b. nothing leaks in, nothing leaks out
@pytest.mark.parametrize("mode", [GELU, RESID, RELU])
@pytest.mark.parametrize("K", [640, 512, 1024, 2048, 4096])
def test_splitk_padding_scratch_guards_determinism(K, mode):
    N, m_valid, M = 384, 77, _rows_M(mode)
    S = K_TABLE[K][0]
    assert _plan_splitk(M, N, K, mode, m_valid) == S
    need = _need(M, m_valid, N, K)
    assert need == S * 128 * N * 4
    p = _problem(M, N, K)
    A0 = p["A"].clone()
    A0[m_valid:] = 0
    sk, sk_can = _guarded(need, torch.float32, 0.0)
    base, can = _run_rows(p, M, m_valid, N, K, mode, True, sk, need, A=A0)
    assert _intact(can) and _intact(sk_can)
    _assert_rows(base, p, m_valid, mode, True)
    base_bits = base[:m_valid].clone().view(torch.int16 if base.dtype == torch.bfloat16 else torch.int32)

    def same(out):
        return torch.equal(out[:m_valid].view(base_bits.dtype), base_bits)

    # the same call again
    again, can = _run_rows(p, M, m_valid, N, K, mode, True, sk, need, A=A0)
    assert same(again) and _intact(can) and _intact(sk_can)
    # NaN in the padding rows of A stays in the padding rows
    An = p["A"].clone()
    An[m_valid:] = float("nan")
    padded, can = _run_rows(p, M, m_valid, N, K, mode, True, sk, need, A=An)
    assert same(padded) and _intact(can) and _intact(sk_can)
    # whatever the scratch held before the call is overwritten before it is read
    sk.fill_(float("nan"))
    stale, can = _run_rows(p, M, m_valid, N, K, mode, True, sk, need, A=A0)
    assert same(stale) and _intact(can) and _intact(sk_can)


# ---------------------------------------------------------------- c. the scratch decides the path, not the result
@pytest.mark.parametrize("mode", [GELU, RESID, RELU])
@pytest.mark.parametrize("scratch", ["null", "one_byte_short"])
@pytest.mark.parametrize("N,K,m_valid", [(384, 640, 77), (128, 2048, 128)])
def test_without_enough_scratch_the_tile_path_takes_over(N, K, m_valid, scratch, mode):
    M = _rows_M(mode)
    need = _need(M, m_valid, N, K)
    assert need == K_TABLE[K][0] * 128 * N * 4
    p = _problem(M, N, K)
    if scratch == "null":
        out, can = _run_rows(p, M, m_valid, N, K, mode, True, None, 0)
    else:
        sk, sk_can = _guarded(need, torch.float32, float("nan"))
        out, can = _run_rows(p, M, m_valid, N, K, mode, True, sk, need - 1)
        assert torch.isnan(sk).all() and _intact(sk_can)      # nothing was written to a scratch that is too small
    assert _intact(can)
    _assert_rows(out, p, m_valid, mode, True)


@pytest.mark.parametrize("mode", [GELU, RESID, RELU])
def test_k448_is_not_a_split_shape(mode):
    """K < 512 and K % 128 != 0: no slices, no scratch bytes, and the call is still right (given a scratch it leaves alone)"""
    M, N, K, m_valid = _rows_M(mode), 384, 448, 77
    assert _plan_splitk(M, N, K, mode, m_valid) == 0 and _need(M, m_valid, N, K) == 0
    p = _problem(M, N, K)
    sk, sk_can = _guarded(1 << 20, torch.float32, float("nan"))
    out, can = _run_rows(p, M, m_valid, N, K, mode, True, sk, 1 << 20)
    assert torch.isnan(sk).all() and _intact(sk_can) and _intact(can)
    _assert_rows(out, p, m_valid, mode, True)


# ---------------------------------------------------------------- d. fused reduction + residual + LayerNorm
@functools.lru_cache(maxsize=None)
def _ln_problem(N, K, with_bias):
    """x, ln_w, ln_b of one shape and the float64 references of the residual row and its LayerNorm (M = 128)"""
    p = _problem(128, N, K)
    g = torch.Generator().manual_seed(7919 * N + K)
    x = torch.randn(128, N, generator=g)
    ln_w = 1 + 0.1 * torch.randn(N, generator=g)
    ln_b = 0.1 * torch.randn(N, generator=g)
    x_ref = x.double() + p["prod"] + (p["bias64"] if with_bias else 0.0)
    mean = x_ref.mean(-1, keepdim=True)
    rstd = (x_ref.var(-1, unbiased=False, keepdim=True) + EPS).rsqrt()
    h_ref = (x_ref - mean) * rstd * ln_w.double() + ln_b.double()
    return {"x": x, "ln_w": ln_w.cuda(), "ln_b": ln_b.cuda(), "x_ref": x_ref, "h_ref": h_ref, "rstd": rstd.squeeze(-1),
            "w_max": ln_w.abs().max().item()}


def _run_resid_ln(N, K, m_valid, ln_rows, post_ln, with_bias, sk, sk_bytes):
    p, q = _problem(128, N, K), _ln_problem(N, K, with_bias)
    x, x_can = _guarded(128 * N * 4, torch.float32)
    x = x.view(128, N)
    x.copy_(q["x"])
    h, h_can = _guarded(128 * N * 2, torch.int16, 0x7FC1)      # a NaN pattern no kernel produces
    h = h.view(128, N)
    _ok(_dbg().wise_debug_gemm_resid_ln_rows(p["A"].data_ptr(), p["W"].data_ptr(), p["bias"].data_ptr() if with_bias else None,
                                             128, m_valid, ln_rows, N, K, x.data_ptr(), q["ln_w"].data_ptr(), q["ln_b"].data_ptr(),
                                             EPS, post_ln, h.data_ptr(), None if sk is None else sk.data_ptr(), sk_bytes,
                                             _lib.stream_ptr()), "gemm_resid_ln_rows")
    torch.cuda.synchronize()
    assert _intact(x_can) and _intact(h_can)
    return x, h


def _assert_resid_ln(x, h, N, K, ln_rows, post_ln, with_bias):
    """the float64 bounds on rows < ln_rows"""
    q = _ln_problem(N, K, with_bias)
    x_ref, h_ref = q["x_ref"][:ln_rows], q["h_ref"][:ln_rows]
    got_x = x[:ln_rows].cpu().double()
    got_h = h[:ln_rows].view(torch.bfloat16).float().cpu()
    assert torch.isfinite(got_x).all() and torch.isfinite(got_h).all()
    if post_ln:
        tol_x = F32_TOL * q["w_max"] * q["rstd"][:ln_rows].max().item() + 1e-5
        err_x = (got_x - h_ref).abs().max().item()
    else:
        tol_x = F32_TOL
        err_x = (got_x - x_ref).abs().max().item()
    tol_h = 2.0 ** -7 * h_ref.abs().max().item()
    err_h = (got_h - bf16_round(h_ref.float())).abs().max().item()
    print(f"x: max error {err_x:.3e} (bound {tol_x:.3e});  h: max error {err_h:.3e} (bound {tol_h:.3e})")
    assert err_x <= tol_x
    assert err_h <= tol_h


def _bf16_steps(a, b):
    """how many bf16 values lie between the elements of two int16 bit images (0: the same value)"""
    def key(t):
        t = t.cpu().to(torch.int32)
        return torch.where(t >= 0, t, -(t & 0x7FFF))
    return (key(a) - key(b)).abs()


LN_SHAPES = [(N, K) for N in (256, 768, 1024, 1280) for K in (640, 512, 1024)] + [(2048, 1024), (3072, 1024), (4096, 1024)]


def _ln_cases():
    """every shape x post_ln, two cases each: m_valid walks 1 / 77 / 128 and the bias comes and goes"""
    out = []
    for si, (N, K) in enumerate(LN_SHAPES):
        for post_ln in (0, 1):
            i = 2 * si + post_ln
            for j in range(2):
                mv = M_VALID[(i + j) % 3]
                with_bias = j == i % 2
                out.append(pytest.param(N, K, mv, post_ln, with_bias,
                                        id=f"N{N}-K{K}-mv{mv}-{'post' if post_ln else 'pre'}-{'bias' if with_bias else 'nobias'}"))
    return out


def test_fused_ln_cases_cover_every_nv_and_every_loop_shape():
    """NV = 1..4, a full and a partial last column group of 256 float4, and S = 2 (tail loop only), 4 (one unrolled pass),
    >= 8 (several passes) of the four-way unrolled partial-sum loop — S as the plan gives it"""
    nv = {((N // 4 + 255) // 256, N // 4 % 256 == 0) for N, _ in LN_SHAPES}
    assert {(1, False), (1, True), (2, False), (2, True)} <= nv and {n for n, _ in nv} == {1, 2, 3, 4}
    for N in (256, 768, 1024, 1280):
        assert [_plan_splitk(128, N, K, RESID, 77) for K in (640, 512, 1024)] == [2, 4, 8]
    assert _plan_splitk(128, 4096, 1024, RESID, 77) == 8 and _need(128, 77, 4096, 1024) == 16 << 20
    assert {c.values[2] for c in _ln_cases()} == set(M_VALID)


def _fused(N, K, m_valid, post_ln, with_bias):
    """one fused call on a NaN-filled scratch of exactly the size the plan asks for: (x, h, scratch, its size)"""
    S = _plan_splitk(128, N, K, RESID, m_valid)
    need = _need(128, m_valid, N, K)
    assert S >= 2 and need == S * 128 * N * 4
    sk, sk_can = _guarded(need, torch.float32, float("nan"))
    x, h = _run_resid_ln(N, K, m_valid, m_valid, post_ln, with_bias, sk, need)
    assert _intact(sk_can)
    assert not torch.isnan(sk).any()      # all S partial tiles were written: the split path ran, and with S slices
    return x, h, sk, need


@pytest.mark.parametrize("N,K,m_valid,post_ln,with_bias", _ln_cases())
def test_fused_reduce_ln(N, K, m_valid, post_ln, with_bias):
    """gemm_splitk_kernel<4> + splitk_reduce_ln_kernel<NV> against float64"""
    x, h, _, _ = _fused(N, K, m_valid, post_ln, with_bias)
    _assert_resid_ln(x, h, N, K, m_valid, post_ln, with_bias)
    # the rows beyond m_valid are nobody's: one workgroup per row of data
    q = _ln_problem(N, K, with_bias)
    assert torch.equal(x[m_valid:].cpu(), q["x"][m_valid:]) and bool((h[m_valid:] == 0x7FC1).all().item())


@pytest.mark.parametrize("N,K,m_valid,post_ln,with_bias", [c for c in _ln_cases() if c.values[3] == 0])
def test_fused_reduce_ln_against_the_launches_it_replaces(N, K, m_valid, post_ln, with_bias):
    """Pre-LN, on the same scratch: x bit-equal to the split-K residual GEMM (mode 3), h within one bf16 ulp, element by
    element, of wise_layernorm_f32_bf16 of that x.

    What an MI355X gave: x and h both bit-equal in all 30 cases, which is what the comment on gemm_resid_ln_rows promises
    and what the last assertion holds the kernels to.  (With the fused kernel's earlier statistics — wave sums, then the
    four waves' sums — x was bit-equal and h was not: up to 5 elements of a case's m_valid * N sat on the neighbouring bf16
    value, and in N4096-K1024-mv77-pre-bias one element that ln_b cancels to 9e-7 was four bf16 values away, 1.6e-8 in
    fp32.  The fused kernel now sums the statistics in layernorm_kernel's order.)"""
    assert post_ln == 0
    x, h, sk, need = _fused(N, K, m_valid, 0, with_bias)
    p, q = _problem(128, N, K), _ln_problem(N, K, with_bias)
    x2 = q["x"].cuda()
    _ok(_dbg().wise_debug_gemm_rows(p["A"].data_ptr(), p["W"].data_ptr(), p["bias"].data_ptr() if with_bias else None, 128,
                                    m_valid, N, K, RESID, x2.data_ptr(), sk.data_ptr(), need, _lib.stream_ptr()), "gemm_rows")
    h2 = torch.full((128, N), 0x7FC1, dtype=torch.int16, device="cuda")
    _ok(_dbg().wise_layernorm_f32_bf16(x2.data_ptr(), q["ln_w"].data_ptr(), q["ln_b"].data_ptr(), m_valid, N, EPS, h2.data_ptr(),
                                       _lib.stream_ptr()), "layernorm")
    torch.cuda.synchronize()
    assert torch.equal(x.view(torch.int32), x2.view(torch.int32))
    steps = _bf16_steps(h[:m_valid], h2[:m_valid])
    print(f"h: {int((steps != 0).sum())} of {steps.numel()} elements differ from the unfused LayerNorm, by at most {int(steps.max())} bf16 value(s)")
    assert int(steps.max()) <= 1
    assert torch.equal(h[:m_valid], h2[:m_valid])


@pytest.mark.parametrize("N,K", LN_SHAPES)
def test_fused_post_ln_gives_the_bits_of_layernorm_dual(N, K):
    """Post-LN: with ln_rows = m_valid - 1 the same call runs the split-K residual GEMM and layernorm_f32_dual (xo == x);
    the rows both forms normalise come out with the same fp32 x and the same bf16 h."""
    x, h, sk, need = _fused(N, K, 128, 1, True)
    x2, h2 = _run_resid_ln(N, K, 128, 127, 1, True, sk, need)
    assert torch.equal(x[:127].view(torch.int32), x2[:127].view(torch.int32))
    assert torch.equal(h[:127], h2[:127])


@pytest.mark.parametrize("post_ln", [0, 1])
@pytest.mark.parametrize("how", ["ln_rows_below_m_valid", "no_scratch"])
def test_resid_ln_falls_back_to_two_launches(how, post_ln):
    """Not the fused kernel: the residual GEMM, then layernorm_f32_bf16 or (post_ln) layernorm_f32_dual with xo == x"""
    N, K = 768, 640
    if how == "ln_rows_below_m_valid":
        m_valid, ln_rows = 64, 50
        need = _need(128, m_valid, N, K)
        assert need == 2 * 128 * N * 4
        sk, sk_can = _guarded(need, torch.float32, float("nan"))
        x, h = _run_resid_ln(N, K, m_valid, ln_rows, post_ln, True, sk, need)
        assert _intact(sk_can)
        # the rows between ln_rows and m_valid took the GEMM and no LayerNorm
        q = _ln_problem(N, K, True)
        assert (x[ln_rows:m_valid].cpu().double() - q["x_ref"][ln_rows:m_valid]).abs().max().item() <= F32_TOL
        assert bool((h[ln_rows:] == 0x7FC1).all().item())
    else:
        m_valid = ln_rows = 77
        x, h = _run_resid_ln(N, K, m_valid, ln_rows, post_ln, True, None, 0)
    _assert_resid_ln(x, h, N, K, ln_rows, post_ln, True)


def test_resid_ln_n128_pre_ln_is_served():
    """N = 128 is too narrow for the fused kernel; the pre-LN form runs the two launches (narrow LayerNorm)"""
    N, K, m_valid = 128, 640, 77
    need = _need(128, m_valid, N, K)
    assert need == 2 * 128 * N * 4
    sk, _ = _guarded(need, torch.float32, float("nan"))
    x, h = _run_resid_ln(N, K, m_valid, m_valid, 0, True, sk, need)
    _assert_resid_ln(x, h, N, K, m_valid, 0, True)


@pytest.mark.parametrize("N,K,post_ln", [(128, 640, 1), (4096 + 128, 512, 0), (4096 + 128, 512, 1)])
def test_resid_ln_refuses_a_width_the_layernorm_cannot_take_before_it_touches_x(N, K, post_ln):
    """post-LN needs N > 128 (layernorm_f32_dual), every LayerNorm N <= 4096: refused before the GEMM accumulates into x"""
    d = _dbg()
    m_valid = 77
    g = torch.Generator().manual_seed(N + K)
    A = torch.randn(128, K, generator=g).to(torch.bfloat16).cuda()
    W = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16).cuda()
    x0 = torch.randn(128, N, generator=g)
    x = x0.cuda()
    ln = torch.ones(N, device="cuda")
    h = torch.full((128, N), 0x7FC1, dtype=torch.int16, device="cuda")
    need = max(_need(128, m_valid, N, K), 4)
    sk = torch.full((need // 4,), float("nan"), device="cuda")
    rc = d.wise_debug_gemm_resid_ln_rows(A.data_ptr(), W.data_ptr(), None, 128, m_valid, m_valid, N, K, x.data_ptr(), ln.data_ptr(),
                                         ln.data_ptr(), EPS, post_ln, h.data_ptr(), sk.data_ptr(), need, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0
    msg = d.wise_last_error().decode()
    assert "gemm_resid_ln" in msg and f"N={N}" in msg, msg
    assert torch.equal(x.cpu().view(torch.int32), x0.view(torch.int32))
    assert bool((h == 0x7FC1).all().item()) and torch.isnan(sk).all()


# ---------------------------------------------------------------- e. refusals without a launch
@pytest.mark.parametrize("what", ["null_A", "null_Wt", "null_out", "M_192", "K_528", "mode_7"])
def test_gemm_rows_refuses_without_a_launch(what):
    d = _dbg()
    M, N, K, mode, m_valid = 128, 128, 640, BF16, 77
    if what == "M_192":
        M = 192
    elif what == "K_528":
        K = 528
    elif what == "mode_7":
        mode = 7
    A = torch.ones(256, 640, dtype=torch.bfloat16, device="cuda")
    W = torch.ones(128, 640, dtype=torch.bfloat16, device="cuda")
    out = torch.full((256, 128), 0x7FC1, dtype=torch.int32, device="cuda")     # room for an fp32 result of 256 rows
    sk = torch.full((32 * 128 * 128,), float("nan"), device="cuda")
    rc = d.wise_debug_gemm_rows(None if what == "null_A" else A.data_ptr(), None if what == "null_Wt" else W.data_ptr(), None,
                                M, m_valid, N, K, mode, None if what == "null_out" else out.data_ptr(), sk.data_ptr(),
                                sk.numel() * 4, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0
    assert "gemm_bf16" in d.wise_last_error().decode()
    assert bool((out == 0x7FC1).all().item()) and torch.isnan(sk).all()

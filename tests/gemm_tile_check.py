"""The checker of tests/test_gpu_gemm_tiles.py: an output against the exact pre-activation through an epilogue mode.  Plain
torch on whatever device the tensors sit on, so tests/test_gemm_tile_cases_cpu.py can hold it to made-up wrong outputs."""
import torch

from tests import gemm_tile_cases as gc


def act64(pre, mode):
    """the float64 activation of modes 1, 2, 5"""
    pre = pre.double()
    if mode == gc.QUICKGELU:
        return pre * torch.sigmoid(1.702 * pre)
    if mode == gc.GELU:
        return 0.5 * pre * (1 + torch.erf(pre / 2 ** 0.5))
    assert mode == gc.GELU_TANH
    return 0.5 * pre * (1 + torch.tanh(0.7978845608028654 * (pre + 0.044715 * pre ** 3)))


def where(bad, what):
    idx = bad.nonzero()
    r, c = (int(x) for x in idx[0])
    return f"{what}: {idx.shape[0]} of {bad.numel()} elements differ, the first at row {r}, column {c}"


def assert_epilogue(got, pre, mode, what, resid=None):
    """got against the exact pre-activation `pre` (fp32) through epilogue `mode`: equality for modes 0, 3, 4, 6;
    |got - want| <= 2^-8 |want| + 5e-5 against the float64 activation for modes 1, 2, 5"""
    if mode in (gc.RESID, gc.F32):
        want = pre + resid if mode == gc.RESID else pre
        assert got.dtype == torch.float32
        assert torch.equal(got, want), where(got != want, what)
    elif mode in (gc.BF16, gc.RELU):
        want = (pre.clamp(min=0) if mode == gc.RELU else pre).to(torch.bfloat16)
        assert got.dtype == torch.bfloat16
        assert torch.equal(got, want), where(got != want, what)
    else:
        want = act64(pre, mode)
        err = (got.double() - want).abs()
        tol = 2.0 ** -8 * want.abs() + 5e-5
        print(f"{what}: max |got - want| / bound = {(err / tol).max().item():.3f}")
        assert bool((err <= tol).all()), where(~(err <= tol), what)      # (~(<=): a NaN counts)

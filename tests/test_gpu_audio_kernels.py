"""-m gpu: the audio towers' own kernels one by one against float64 (tests/audio_kernel_ref.py: cases, restatements, checker).

embed_tok_kernel / embed_kernel, swin96_block_attn_kernel<0 | 4>, merge_ln_kernel<2 | 3 | 6> and latent_kernel in both input
forms, proj_ln_norm_kernel (csrc/htsat.hip), conv_block1_kernel and head_pool_kernel (csrc/cnn14.hip), each through its
wise_debug_* twin of the debug library, which calls the launch function the tower calls: grid, block, LDS bytes and template
dispatch are the tower's.  Elementwise bounds, no cosine: fp32 outputs inside 8 x the float32 restatement's own error per row,
bf16 outputs inside half a bf16 step + that, with at most 1 % of the elements not bf16(want64) (a dropped lo half flips a third);
block 1 inside the bf16 convolution's rtol 8e-3 / atol 2e-3; outputs finite, guard rows behind every output untouched, NaN guard
rows behind every input.  tests/test_audio_kernel_ref_cpu.py holds the checker to planted faults.

swin96 is judged by the bf16 noise of the operation itself, n = |rounded - exact| of the two float64 restatements:
max |got - rounded| <= 2 max n and mean |got - rounded| <= 2 mean n, over all rows but two and for the constant row and the
outlier row each by its own n.  Seen on an MI355X (max ratio, mean ratio):

  case (shift, B, grid)    all other rows     constant row       outlier row
  0, 1, 0   and 0, 1, 24   0.362   0.023      0.631   0.652      0.540   0.025
  0, 2, 0                  0.442   0.023      0.194   0.297      0.427   0.016
  4, 1, 0   and 4, 1, 24   0.332   0.025      0.461   0.414      0.693   0.021
  4, 2, 0                  0.433   0.021      0.142   0.141      0.003   0.000
  4, 9, 0                  0.299   0.019      0.705   0.598      0.356   0.011
(24 workgroups of three and two trips give the figures of the tower's grid.)  No ratio reaches 1: the kernel rounds where `rounded` does.

What these tests found when they were written: both embedding kernels took the bicubic fraction from the UNROUNDED product
t * scale (the compiler had contracted src - floorf(src) into one fma) where torch's upsample_bicubic2d and the oracle take it
from the rounded fp32 position, which moved 40 % of the elements at Fc = 601 and 1023 beyond tau_r, by up to 38 and 54 tau_r
(3e-4 absolute); and their Horner-form cubic weights lost 4.5e-7 to cancellation, 1.04 tau_r on one row at Fc = 5.  Both are
fixed in csrc/htsat.hip (bicubic_src, cubic_weights); every embed case now stays under 0.43 tau_r.
"""
import ctypes as C
import functools

import pytest
import torch

from tests import audio_kernel_ref as ak
from wise_amd import _lib

pytestmark = pytest.mark.gpu

_P, _I, _LL = C.c_void_p, C.c_int, C.c_longlong
SIGNATURES = {
    "wise_debug_htsat_embed": [_P, _I, _I, _P, _P, _P, _P, _P, _I, _P],
    "wise_debug_swin96_block_attn": [_P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P],
    "wise_debug_htsat_merge_ln": [_P, _I, _I, _I, _P, _P, _P, _LL, _P],
    "wise_debug_htsat_latent": [_P, _I, _P, _P, _P, _LL, _P],
    "wise_debug_proj_ln_norm": [_P, _I, _P, _P, _P, _P],
    "wise_debug_cnn14_block1": [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P],
    "wise_debug_cnn14_head_pool": [_P, _I, _I, _I, _I, _P, _P],
}


@functools.lru_cache(maxsize=None)
def _dbg():
    d = _lib.load_debug()
    for name, args in SIGNATURES.items():
        fn = getattr(d, name)
        fn.argtypes, fn.restype = args, C.c_int
    return d


@functools.lru_cache(maxsize=None)
def _problem(kernel, key):
    """the references of one data set, built once: forms, grids and chunks that share a shape share them"""
    return ak.build(kernel, dict(key))


def _data_key(c):
    return tuple((k, v) for k, v in c.items() if k not in ("form", "grid", "chunk"))


def _run(kernel, c):
    p = _problem(kernel, _data_key(c))
    p.what = ak.case_id(kernel, c)
    d, st = _dbg(), _lib.stream_ptr()
    dev = {k: v.cuda() for k, v in p.inputs.items()}
    a = lambda k: dev[k].data_ptr()
    out = None if kernel == "swin96" else ak.out_buffer(p.rows, p.cols, p.out_dtype).cuda()
    if kernel == "embed":
        rc = d.wise_debug_htsat_embed(a("mel"), c["B"], c["Fc"], a("pw"), a("pb"), a("lnw"), a("lnb"), out.data_ptr(), c["form"], st)
    elif kernel == "swin96":
        out = dev["x"].reshape(-1, 96)                  # in place: the rows past B*4096 are the guards
        rc = d.wise_debug_swin96_block_attn(a("x"), c["B"], a("n1w"), a("n1b"), a("wqkv"), a("qkvb"), a("relb"), a("wproj"),
                                            a("pb"), c["shift"], c["grid"], st)
    elif kernel == "merge_ln":
        rc = d.wise_debug_htsat_merge_ln(a("x"), c["B"], c["H"], c["C"], a("w"), a("b"), out.data_ptr(), p.lo_off, st)
    elif kernel == "latent":
        rc = d.wise_debug_htsat_latent(a("x"), c["B"], a("nw"), a("nb"), out.data_ptr(), p.lo_off, st)
    elif kernel == "proj_ln_norm":
        rc = d.wise_debug_proj_ln_norm(a("e"), c["B"], a("lw"), a("lb"), out.data_ptr(), st)
    elif kernel == "block1":
        rc = d.wise_debug_cnn14_block1(a("mel"), a("w0"), a("s0"), a("Wt"), a("bias2"), c["B"], c["T"], c["chunk"],
                                       out.data_ptr(), st)
    else:
        rc = d.wise_debug_cnn14_head_pool(a("x"), c["B"], c["T"], c["F"], c["C"], out.data_ptr(), st)
    assert rc == 0, d.wise_last_error().decode()
    torch.cuda.synchronize()
    return ak.check(p, out.cpu())


def _params(kernel):
    return pytest.mark.parametrize("c", ak.CASES[kernel], ids=[ak.case_id(kernel, c) for c in ak.CASES[kernel]])


@_params("embed")
def test_embed(c):
    _run("embed", c)


@_params("swin96")
def test_swin96_block_attn(c):
    _run("swin96", c)


@_params("merge_ln")
def test_merge_ln(c):
    _run("merge_ln", c)


@_params("latent")
def test_latent(c):
    _run("latent", c)


@_params("proj_ln_norm")
def test_proj_ln_norm(c):
    _run("proj_ln_norm", c)


@_params("block1")
def test_block1(c):
    _run("block1", c)


@_params("head_pool")
def test_head_pool(c):
    _run("head_pool", c)


def test_debug_entries_refuse_other_shapes():
    d, st = _dbg(), _lib.stream_ptr()
    p = torch.zeros(64, device="cuda").data_ptr()

    def refused(rc, name):
        assert rc != 0 and name.encode() in d.wise_last_error(), (name, rc, d.wise_last_error())

    for fc, form in ((1, 0), (1025, 0), (601, 2)):
        refused(d.wise_debug_htsat_embed(p, 1, fc, p, p, p, p, p, form, st), "debug_htsat_embed")
    refused(d.wise_debug_htsat_embed(0, 1, 601, p, p, p, p, p, 0, st), "debug_htsat_embed")
    for B, shift, grid in ((0, 0, 0), (1, 2, 0), (1, 0, 513), (1, 4, -1)):
        refused(d.wise_debug_swin96_block_attn(p, B, p, p, p, p, p, p, p, shift, grid, st), "debug_swin96_block_attn")
    for B, H, Cc, lo in ((1, 7, 96, 0), (1, 0, 96, 0), (1, 8, 100, 0), (1, 8, 768, 0), (0, 8, 96, 0), (1, 8, 96, 64), (1, 8, 96, -1)):
        refused(d.wise_debug_htsat_merge_ln(p, B, H, Cc, p, p, p, lo, st), "debug_htsat_merge_ln")
    for B, lo in ((0, 0), (1, 768), (1, -1)):
        refused(d.wise_debug_htsat_latent(p, B, p, p, p, lo, st), "debug_htsat_latent")
    refused(d.wise_debug_proj_ln_norm(p, 0, p, p, p, st), "debug_proj_ln_norm")
    refused(d.wise_debug_proj_ln_norm(p, 1, p, 0, p, st), "debug_proj_ln_norm")
    for B, T, chunk in ((1, 31, 0), (0, 32, 0), (1, 32, -1)):
        refused(d.wise_debug_cnn14_block1(p, p, p, p, p, B, T, chunk, p, st), "debug_cnn14_block1")
    for B, T, Fq, Cc in ((1, 1, 2, 4), (1, 1, 2, 60), (1, 0, 2, 64), (1, 1, 0, 64), (0, 1, 2, 64)):
        refused(d.wise_debug_cnn14_head_pool(p, B, T, Fq, Cc, p, st), "debug_cnn14_head_pool")

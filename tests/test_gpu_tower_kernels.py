"""-m gpu: the image and text towers' own kernels one by one against float64 (tests/tower_kernel_ref.py: cases, restatements, checker).

patchify_kernel / patchify8_kernel<u8 | float>, embed_pos_kernel, embed_lnpre_kernel<NV> plain and fold, cls_ln_kernel<NV> without and
with positions, l2norm_rows_kernel, map_pool_kernel, hilo_rows_kernel, layernorm_kernel<NV> with its fp32 copy (csrc/vit.hip),
text_embed_kernel (csrc/text.hip), xlmr_embed_kernel and xlmr_meanpool_kernel (csrc/xlmr_text.hip), each through its wise_debug_*
twin of the debug library, which calls the launch function the tower calls: grid, block and template dispatch are the tower's.
layernorm_narrow_kernel, layernorm_kernel<NV> and layernorm_rows_kernel<NV, 4> go through the product's wise_layernorm_f32_bf16 on the
shapes and data of tests/test_gpu_row_kernel_hashes.py.  Bit patterns where one rounded operation of the kernel is one of torch
(gathers, sums of two or three terms, integers, the u8 normalisation with its two true divisions); elementwise bounds elsewhere:
fp32 outputs inside 8 x the float32 restatement's own error per row, bf16 outputs inside half a bf16 step + that with at most 1 % of
the elements not bf16(want64); outputs finite, guard rows behind every output and the rows a kernel must leave alone untouched, NaN
guard rows behind every input.  tests/test_tower_kernel_ref_cpu.py holds the checker to planted faults.

Seen on an MI355X (the largest figure over a kernel's cases; 1 = the bound):

  kernel                          output    bits differing   max err / bound   not bf16(want64), at most
  patchify, all four forms        patches   0                                  (fp32 and u8, both sets of constants, offset pointer)
  embed_pos, hilo_rows            x / out   0
  text_embed                      x, eot    0
  xlmr_embed                      x, lens   0
  xlmr_meanpool, first row only   pooled    0
  xlmr_meanpool, mean             pooled                     0.980             0 %
  embed_lnpre, plain              x                          0.200 (tau_r)
  embed_lnpre, fold               hi                         0.981             0 %      hi + lo: 0.433; rstd: 0.111 (tau_r)
  cls_ln                          y                          0.995             0.20 %   (1 element of 512)
  l2norm_rows                     out                        0.103 (tau_r)
  map_pool                        o                          0.970             0.39 %   (1 element of 256)
  layernorm (product entry)       y                          0.996             0.008 %
  layernorm_dual                  xo                         0.176 (tau_r)
  layernorm_dual                  y                          0.994             0.60 %   and y == bf16(xo) everywhere
A bf16 output sits at up to 0.996 of its bound because the bound is half a bf16 step at the worst place of a binade; the fp32
outputs show what the kernels themselves lose: under a fifth of tau_r.  The 0.60 % (32 of 5376 elements; 0.54 % at width 132) is
the row of variance 2^-24 at eps 1e-12 and a width that is no power of two: the fp32 mean of 1.25 +- 2^-12 is off by up to 2^-24,
3e-4 of a deviation, which turns 4 % of that one row's roundings — in the float32 restatement just as much, and at widths 256,
1024 and 4096, where the mean is exact, not at all.

What these tests found when they were written: no kernel outside its bound, and the u8 normalisation bit-equal to two true
divisions for all 256 byte values in every channel under both sets of constants.  Read on the way: the caption head's ln_f ignored
the tower's eps, and text towers wider than 2048 were admitted though the head's LayerNorm cannot hold their rows (both below).
"""
import ctypes as C
import functools

import pytest
import torch

from tests import tower_kernel_ref as tk
from wise_amd import _lib

pytestmark = pytest.mark.gpu

_P, _I, _LL, _F = C.c_void_p, C.c_int, C.c_longlong, C.c_float
SIGNATURES = {
    "wise_debug_vit_patchify": [_P, _I, _I, _I, _I, _I, _I, _P, _P],
    "wise_debug_vit_embed_pos": [_P, _P, _I, _I, _I, _P, _P],
    "wise_debug_vit_embed_lnpre": [_P, _P, _P, _P, _P, _I, _I, _I, _F, _P, _P, _P, _LL, _P],
    "wise_debug_pooled_ln": [_P, _P, _P, _I, _I, _I, _F, _P, _P, _P],
    "wise_debug_l2norm_rows": [_P, _I, _I, _P, _P],
    "wise_debug_vit_map_pool": [_P, _P, _I, _I, _I, _P, _P],
    "wise_debug_vit_hilo_rows": [_P, _LL, _I, _I, _I, _P, _I, _P],
    "wise_debug_layernorm_dual": [_P, _P, _P, _I, _I, _F, _P, _P, _P],
    "wise_debug_text_embed": [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P],
    "wise_debug_xlmr_embed": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P],
    "wise_debug_xlmr_meanpool": [_P, _P, _I, _I, _I, _I, _P, _P],
}

@functools.lru_cache(maxsize=None)
def _dbg():
    d = _lib.load_debug()
    for name, args in SIGNATURES.items():
        fn = getattr(d, name)
        fn.argtypes, fn.restype = args, C.c_int
    return d


def _buffers(p):
    return {name: tk.out_buffer(o.rows, o.cols, o.dtype).cuda() for name, o in p.outs.items()}


def _run(kernel, c):
    p = tk.build(kernel, c)
    d, st = _dbg(), _lib.stream_ptr()
    dev = {k: v.cuda() for k, v in p.inputs.items()}
    a = lambda k: dev[k].data_ptr()
    out = _buffers(p)
    o = lambda k: out[k].data_ptr()
    if kernel == "patchify":
        rc = d.wise_debug_vit_patchify(a("img") + c["off"], _lib.WISE_VIT_IN_U8 if c["inp"] == "u8" else _lib.WISE_VIT_IN_F32, c["B"],
                                       c["S"], c["P"], tk.kpad(c["P"]), c["arch"], o("patches"), st)
    elif kernel == "embed_pos":
        rc = d.wise_debug_vit_embed_pos(a("patch"), a("pos"), c["B"] * c["T"], c["T"], c["W"], o("x"), st)
    elif kernel == "embed_lnpre":
        rows = c["B"] * c["T"]
        if c["fold"]:
            rc = d.wise_debug_vit_embed_lnpre(a("patch"), a("cls"), a("pos"), a("w"), a("b"), rows, c["T"], c["W"], 1e-5, None, o("hilo"),
                                              o("rstd"), p.args["lo_rows"] * c["W"], st)
        else:
            rc = d.wise_debug_vit_embed_lnpre(a("patch"), a("cls"), a("pos"), a("w"), a("b"), rows, c["T"], c["W"], 1e-5, o("x"), None,
                                              None, 0, st)
    elif kernel == "cls_ln":
        rc = d.wise_debug_pooled_ln(a("x"), a("w"), a("b"), c["B"], c["T"], c["W"], 1e-5, a("pos") if c["pos"] else None, o("y"), st)
    elif kernel == "l2norm":
        rc = d.wise_debug_l2norm_rows(a("e"), c["rows"], c["D"], o("out"), st)
    elif kernel == "map_pool":
        rc = d.wise_debug_vit_map_pool(a("kv"), a("qv"), c["B"], c["T"], c["W"], o("o"), st)
    elif kernel == "hilo_rows":
        rc = d.wise_debug_vit_hilo_rows(a("hi"), p.args["lo_off"], c["n"], c["stride"], c["W"], o("out"), c["ostride"], st)
    elif kernel == "layernorm":
        d = _lib.lib()                   # the product's entry
        rc = d.wise_layernorm_f32_bf16(a("x"), a("w"), a("b"), c["rows"], c["W"], 1e-5, o("y"), st)
    elif kernel == "layernorm_dual":
        if c["inplace"]:                 # xo == x: the input's own buffer, its NaN rows the guard
            out["xo"] = dev["x"].reshape(-1, c["W"])
        rc = d.wise_debug_layernorm_dual(a("x"), a("w"), a("b"), c["rows"], c["W"], c["eps"], o("xo"), o("y"), st)
    elif kernel == "text_embed":
        rc = d.wise_debug_text_embed(a("ids"), a("tok"), a("pos"), c["B"], c["T"], c["W"], tk.VOCAB, c["pool"], o("x"), o("eot"), st)
    elif kernel == "xlmr_embed":
        rc = d.wise_debug_xlmr_embed(a("ids"), a("word"), a("pos"), a("type0"), c["B"], c["T"], c["W"], tk.VOCAB, p.args["max_pos"],
                                     c["pad"], c["pos_abs"], o("x"), o("lens"), st)
    else:
        rc = d.wise_debug_xlmr_meanpool(a("x"), a("lens"), c["B"], c["T"], c["W"], c["first"], o("pooled"), st)
    assert rc == 0, d.wise_last_error().decode()
    torch.cuda.synchronize()
    got = {name: t.cpu() for name, t in out.items()}
    figs = {name: tk.check(p, name, got[name]) for name in p.outs}
    if kernel == "layernorm_dual":       # y is the rounding of the row the kernel wrote to xo
        rows = c["rows"]
        same = got["y"][:rows].view(torch.int16) == got["xo"][:rows].to(torch.bfloat16).view(torch.int16)
        assert bool(same.all()), tk.where(~same, p.what + " (y is not bf16(xo))")
    return figs


def _params(kernel):
    return pytest.mark.parametrize("c", tk.CASES[kernel], ids=[tk.case_id(kernel, c) for c in tk.CASES[kernel]])


@_params("patchify")
def test_patchify(c):
    _run("patchify", c)


@_params("embed_pos")
def test_embed_pos(c):
    _run("embed_pos", c)


@_params("embed_lnpre")
def test_embed_lnpre(c):
    _run("embed_lnpre", c)


@_params("cls_ln")
def test_cls_ln(c):
    _run("cls_ln", c)


@_params("l2norm")
def test_l2norm_rows(c):
    _run("l2norm", c)


@_params("map_pool")
def test_map_pool(c):
    _run("map_pool", c)


@_params("hilo_rows")
def test_hilo_rows(c):
    _run("hilo_rows", c)


@_params("layernorm")
def test_layernorm(c):
    _run("layernorm", c)


@_params("layernorm_dual")
def test_layernorm_dual(c):
    _run("layernorm_dual", c)


@_params("text_embed")
def test_text_embed(c):
    _run("text_embed", c)


@_params("xlmr_embed")
def test_xlmr_embed(c):
    _run("xlmr_embed", c)


@_params("xlmr_meanpool")
def test_xlmr_meanpool(c):
    _run("xlmr_meanpool", c)


def test_debug_entries_refuse_other_shapes():
    """a null pointer, a width the kernel does not serve, more tokens than the pool holds: an error that names the entry, no launch"""
    d, st = _dbg(), _lib.stream_ptr()
    p = torch.zeros(64, device="cuda").data_ptr()
    U8, F32 = _lib.WISE_VIT_IN_U8, _lib.WISE_VIT_IN_F32

    def refused(rc, name):
        assert rc != 0 and name.encode() in d.wise_last_error(), (name, rc, d.wise_last_error())

    refused(d.wise_debug_vit_patchify(None, U8, 1, 16, 8, 192, 0, p, st), "debug_vit_patchify")
    for S, P, Kp, arch, kind in ((16, 7, 192, 0, U8), (16, 8, 128, 0, U8), (16, 8, 192, 2, U8), (16, 8, 192, 0, 2), (28, 14, 588, 0, F32)):
        refused(d.wise_debug_vit_patchify(p, kind, 1, S, P, Kp, arch, p, st), "debug_vit_patchify")
    refused(d.wise_debug_vit_embed_pos(p, None, 4, 2, 128, p, st), "debug_vit_embed_pos")
    refused(d.wise_debug_vit_embed_pos(p, p, 4, 2, 130, p, st), "debug_vit_embed_pos")
    refused(d.wise_debug_vit_embed_lnpre(p, p, p, p, p, 10, 5, 768, 1e-5, None, None, None, 0, st), "debug_vit_embed_lnpre")
    refused(d.wise_debug_vit_embed_lnpre(p, p, p, p, p, 10, 5, 768, 1e-5, None, p, None, 128 * 768, st), "debug_vit_embed_lnpre")
    for rows, W, lo in ((10, 2052, 0), (10, 770, 0), (11, 768, 0)):
        refused(d.wise_debug_vit_embed_lnpre(p, p, p, p, p, rows, 5, W, 1e-5, p, None, None, lo, st), "debug_vit_embed_lnpre")
    refused(d.wise_debug_vit_embed_lnpre(p, p, p, p, p, 10, 5, 768, 1e-5, None, p, p, 10 * 768 - 4, st), "debug_vit_embed_lnpre")
    refused(d.wise_debug_pooled_ln(p, p, None, 2, 5, 768, 1e-5, None, p, st), "debug_pooled_ln")
    for W in (2052, 4096, 766):
        refused(d.wise_debug_pooled_ln(p, p, p, 2, 5, W, 1e-5, None, p, st), "debug_pooled_ln")
    refused(d.wise_debug_l2norm_rows(p, 2, 64, None, st), "debug_l2norm_rows")
    refused(d.wise_debug_l2norm_rows(p, 2, 0, p, st), "debug_l2norm_rows")
    refused(d.wise_debug_vit_map_pool(p, None, 2, 64, 128, p, st), "debug_vit_map_pool")
    for T, W in ((1025, 128), (0, 128), (64, 96)):
        refused(d.wise_debug_vit_map_pool(p, p, 2, T, W, p, st), "debug_vit_map_pool")
    refused(d.wise_debug_vit_hilo_rows(None, 1024, 1, 1, 64, p, 1, st), "debug_vit_hilo_rows")
    for lo, W in ((63, 64), (1 << 20, 4100)):
        refused(d.wise_debug_vit_hilo_rows(p, lo, 1, 1, W, p, 1, st), "debug_vit_hilo_rows")
    refused(d.wise_debug_layernorm_dual(p, p, p, 2, 256, 1e-5, None, p, st), "debug_layernorm_dual")
    for W in (128, 258, 4100):
        refused(d.wise_debug_layernorm_dual(p, p, p, 2, W, 1e-5, p, p, st), "debug_layernorm_dual")
    refused(d.wise_debug_text_embed(p, p, p, 1, 8, 128, 64, 0, p, None, st), "debug_text_embed")
    for T, W, pool in ((129, 128, 0), (8, 130, 0), (8, 128, 3)):
        refused(d.wise_debug_text_embed(p, p, p, 1, T, W, 64, pool, p, p, st), "debug_text_embed")
    refused(d.wise_debug_xlmr_embed(p, p, p, None, 1, 8, 256, 64, 11, 1, 0, p, p, st), "debug_xlmr_embed")
    for T, W, max_pos, pad in ((129, 256, 200, 1), (8, 258, 11, 1), (8, 256, 9, 1), (8, 256, 11, 64)):
        refused(d.wise_debug_xlmr_embed(p, p, p, p, 1, T, W, 64, max_pos, pad, 0, p, p, st), "debug_xlmr_embed")
    refused(d.wise_debug_xlmr_meanpool(p, None, 1, 8, 256, 0, p, st), "debug_xlmr_meanpool")
    for T, W, first in ((129, 256, 0), (8, 258, 0), (8, 256, 2)):
        refused(d.wise_debug_xlmr_meanpool(p, p, 1, T, W, first, p, st), "debug_xlmr_meanpool")


def test_caption_head_normalises_the_pooled_row_with_the_towers_eps():
    """csrc/text.hip, head 1 (the msclap Projection head) on a tower with eps 1e-6: ln_f of the pooled row takes the tower's eps
    (it took 1e-5 whatever the tower said; no shipped tower sets both).  A layers = 0 tower whose pooled rows are constant up to
    noise of variance 1e-6, so that rstd is 707 with 1e-6 and 301 with 1e-5, against the float64 restatement rounded to bf16
    where the head rounds (the LayerNorm's output and gelu(e1), the GEMM operands).  Bound: 2^-10 of the row's largest element.
    The restatement's own roundings leave fp32 noise; a bf16 rounding of an operand that falls the other way in fp32 moves an
    output by 2^-8 of one of its 128 or 1024 terms, under 2^-11 of the row's scale — the bound allows two.  Seen on an MI355X: 0.365
of the bound; the same restatement with 1e-5 lies 212 bounds away."""
    from oracle.vit_ref import gelu
    from tests.audio_kernel_ref import layer_norm
    from wise_amd.feature.clap_text import pack_caption_weights, random_caption_state_dict
    from wise_amd.feature.text import TextEngine, TextSpec

    T, W = 8, 128
    spec = TextSpec("rows", W, 2, 0, 1024, context=T, vocab=32, act="gelu_new", pool="last_nonzero", head="clap", ln_eps=1e-6)
    sd = random_caption_state_dict(spec, 3, positions=T)
    g = torch.Generator().manual_seed(9)
    tok = torch.tensor([[30, 0, 0, 0, 0, 0, 0, 0], [4, 5, 29, 0, 0, 0, 0, 0], [4, 5, 6, 7, 8, 9, 10, 28]], dtype=torch.int32)
    for b, (tid, at, level) in enumerate(((30, 0, 0.75), (29, 2, 0.75), (28, 7, -0.5))):
        sd["base.wte.weight"][tid] = level - sd["base.wpe.weight"][at] + 1e-3 * torch.randn(W, generator=g)
    eng = TextEngine(spec, sd, max_batch=3, pack=pack_caption_weights)
    assert eng.cfg.eps_e6 == 1 and eng.cfg.head == 1
    got = eng.forward(tok).cpu().double()

    bf = lambda t: t.float().to(torch.bfloat16).double()
    x = (sd["base.wte.weight"][tok.long()] + sd["base.wpe.weight"][:T]).double()             # one fp32 sum, as the kernel's
    pooled = x[torch.arange(3), torch.tensor([0, 2, 7])]

    def head(eps):
        h = bf(layer_norm(pooled, sd["base.ln_f.weight"], sd["base.ln_f.bias"], eps))
        e1 = h @ bf(sd["projection.linear1.weight"]).t()
        e = e1 + bf(gelu(e1)) @ bf(sd["projection.linear2.weight"]).t()
        y = layer_norm(e, sd["projection.layer_norm.weight"], sd["projection.layer_norm.bias"])
        return y / y.norm(dim=-1, keepdim=True)

    want, other = head(1e-6), head(1e-5)
    tol = 2.0 ** -10 * want.abs().amax(dim=1, keepdim=True)
    err = (got - want).abs()
    print(f"caption head, eps 1e-6: max |got - want64| / bound = {float((err / tol).max()):.3f}; "
          f"the 1e-5 restatement is {float(((other - want).abs() / tol).amax()):.0f} bounds away")
    assert bool(((other - want).abs().amax(dim=1, keepdim=True) > 10 * tol).all())           # the rows do tell the two apart
    assert bool((err <= tol).all()), tk.where(~(err <= tol), "caption head, eps 1e-6")


def test_text_towers_refuse_a_width_the_head_cannot_normalise():
    """text_dims: the pooled LayerNorm of the head serves rows of up to 2048 floats; a wider tower is refused before it runs"""
    lib = _lib.load()
    cfg = _lib.TextConfig(77, 1000, 2176, 1, 34, 4 * 2176, 512, 0, 0, 0, 0, 0)
    assert lib.wise_text_layout(C.byref(cfg), None, None) != 0
    assert b"2048" in lib.wise_last_error() and b"2176" in lib.wise_last_error()
    assert lib.wise_text_workspace_bytes(C.byref(cfg), 1) == 0
    ok = _lib.TextConfig(77, 1000, 2048, 1, 32, 4 * 2048, 512, 0, 0, 0, 0, 0)
    assert lib.wise_text_layout(C.byref(ok), None, None) == 0

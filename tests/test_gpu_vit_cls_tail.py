"""-m gpu: the last block of a folded image tower computed for the class rows only (vit.hip transformer_blocks_fold, `tail`).

The tower returns ln_post(x[class row]) @ proj, so after the last block's QKV GEMM only the class query and the class rows
matter.  The class-query form of attention_kernel must give row 0 of the full attention bit for bit, and the whole tower must
give the same embeddings — and the same class rows through the parity tap — as with the full last block, which the debug
library restores with wise_debug_set_vit_cls_tail(0)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import vit_ref
from wise_amd import _lib
from wise_amd.feature.vit import VitEngine, VitSpec, checkpoint_like_state_dict, random_state_dict, spec_for

pytestmark = pytest.mark.gpu

_P = C.c_void_p


def _dbg():
    d = _lib.load_debug()
    d.wise_debug_attention_cls_bf16.argtypes = [_P, C.c_int, C.c_int, C.c_int, _P, _P]
    d.wise_debug_attention_cls_bf16.restype = C.c_int
    d.wise_debug_set_vit_cls_tail.argtypes = [C.c_int]
    d.wise_debug_set_vit_cls_tail.restype = C.c_int
    return d


def _check_dbg(d, rc, what):
    if rc != 0:
        raise RuntimeError(f"debug library {what} failed (rc={rc}): {d.wise_last_error().decode()}")


@pytest.mark.parametrize("B", [1, 37, 256])
@pytest.mark.parametrize("T", [2, 17, 50, 64])
def test_class_attention_is_row_0_of_the_full_attention(B, T):
    H, W = 12, 768
    d = _dbg()
    g = torch.Generator().manual_seed(1000 * B + T)
    qkv = (torch.randn(B * T, 3 * W, generator=g) * 1.5).to(torch.bfloat16).cuda()
    full = torch.empty(B * T, W, dtype=torch.bfloat16, device="cuda")
    _lib.check(_lib.lib().wise_attention_bf16(qkv.data_ptr(), B, T, H, full.data_ptr(), _lib.stream_ptr()), "wise_attention_bf16")
    cls = torch.empty(B, W, dtype=torch.bfloat16, device="cuda")
    _check_dbg(d, d.wise_debug_attention_cls_bf16(qkv.data_ptr(), B, T, H, cls.data_ptr(), _lib.stream_ptr()), "attention_cls")
    torch.cuda.synchronize()
    assert torch.equal(cls.view(torch.int16), full.view(B, T, W)[:, 0].view(torch.int16))


def _debug_forward(eng, x, kind, B, single, tail):
    d = _dbg()
    d.wise_debug_set_vit_cls_tail(1 if tail else 0)
    try:
        out = torch.empty(B, eng.spec.embed_dim, dtype=torch.float32, device="cuda")
        fn = d.wise_vit_forward_single if single else d.wise_vit_forward
        _check_dbg(d, fn(C.byref(eng.cfg), eng.wb.data_ptr(), eng.pf.data_ptr(), x.data_ptr(), kind, B, out.data_ptr(),
                         eng._ws.data_ptr(), eng._ws.numel(), _lib.stream_ptr()), "wise_vit_forward")
        tap = torch.empty(B * eng.spec.tokens, eng.spec.width, dtype=torch.float32, device="cuda")
        _check_dbg(d, d.wise_vit_tap_residual(C.byref(eng.cfg), B, eng._ws.data_ptr(), tap.data_ptr(), _lib.stream_ptr()),
                   "wise_vit_tap_residual")
        torch.cuda.synchronize()
        return out.cpu(), tap.cpu().view(B, eng.spec.tokens, eng.spec.width)
    finally:
        d.wise_debug_set_vit_cls_tail(1)


def _frames(B, S, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(B, 3, S, S), dtype=np.uint8))


def _compare_tower(eng, batches, seed, tail_runs=True):
    """tail_runs: whether the class-row tail applies to this tower (head dim 64); if it does, the tap's non-class rows must
    differ from the full last block's (they keep block L-2's output, plus the attention half with ln_fold = 2) — proof that
    the compact path ran; if it does not, the whole tap equals the full block's"""
    spec = eng.spec
    for B in batches:
        u8 = _frames(B, spec.image_size, seed + B)
        for images in (u8, vit_ref.normalize_u8(u8)):
            x, kind = eng._check_images(images)
            want = eng.forward(images).cpu()                                   # the product library
            want_tap = eng.residual(B).cpu().view(B, spec.tokens, spec.width)
            for single in (True, False):
                on, tap_on = _debug_forward(eng, x, kind, B, single, tail=True)
                off, tap_off = _debug_forward(eng, x, kind, B, single, tail=False)
                assert torch.equal(on, off), (spec.name, spec.ln_fold, B, images.dtype, single)
                assert torch.equal(on, want), (spec.name, spec.ln_fold, B, images.dtype, single)
                assert torch.equal(tap_on[:, 0], tap_off[:, 0]), (spec.name, spec.ln_fold, B, images.dtype, single)
                assert torch.equal(tap_on, want_tap)
                if tail_runs:
                    assert not torch.equal(tap_on[:, 1:], tap_off[:, 1:]), (spec.name, spec.ln_fold, B, "the tail did not run")
                else:
                    assert torch.equal(tap_on, tap_off), (spec.name, spec.ln_fold, B)


@pytest.mark.parametrize("fold", [1, 2])
@pytest.mark.parametrize("weights", ["seeded", "checkpoint_like"])
def test_b32_tower_equals_the_full_last_block(fold, weights):
    spec = spec_for("ViT-B-32", "openai")
    sd = (random_state_dict if weights == "seeded" else checkpoint_like_state_dict)(spec, 11)
    eng = VitEngine(spec, sd, max_batch=256, ln_fold=fold)
    assert eng.spec.ln_fold == fold
    _compare_tower(eng, (1, 37, 256), seed=fold * 7)


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("fold", [1, 2])
def test_short_towers(layers, fold):
    """layers = 1: the first block is the last one (its QKV GEMM reads the rows embed_lnpre_kernel wrote)"""
    spec = VitSpec(f"b32_l{layers}", 224, 32, 768, layers, 12, 3072, 512)
    eng = VitEngine(spec, random_state_dict(spec, 5 + layers), max_batch=64, ln_fold=fold)
    _compare_tower(eng, (1, 37), seed=layers)


def test_narrow_tower_with_gelu():
    """other widths (256, 4 heads, 25 tokens), mlp 2 x width and the erf GELU: the compact regions are carved per shape"""
    spec = VitSpec("narrow", 160, 32, 256, 2, 4, 512, 128, "gelu")
    eng = VitEngine(spec, random_state_dict(spec, 9), max_batch=200, ln_fold=1)
    assert eng.spec.ln_fold == 1
    _compare_tower(eng, (3, 200), seed=3)


def test_head_dim_80_runs_the_full_last_block():
    """the class-query attention is head dim 64 only: a folded tower with head dim 80 (ViT-H/14's; here W = 640, 8 heads) keeps
    the full last block, and its embeddings stay those of the unfolded tower"""
    spec = VitSpec("h80_fold", 126, 14, 640, 2, 8, 1280, 64)
    sd = random_state_dict(spec, 13)
    eng = VitEngine(spec, sd, max_batch=64, ln_fold=1)
    assert eng.spec.ln_fold == 1
    _compare_tower(eng, (1, 37), seed=80, tail_runs=False)
    frames = _frames(37, spec.image_size, 81)
    ref = VitEngine(spec, sd, max_batch=64, ln_fold=0).forward(frames).double().cpu()
    got = eng.forward(frames).double().cpu()
    cos = ((got * ref).sum(-1) / (got.norm(dim=-1) * ref.norm(dim=-1))).min().item()
    assert cos >= 1 - 1e-3, cos

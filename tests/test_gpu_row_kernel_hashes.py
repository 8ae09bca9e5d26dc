"""-m gpu: the LayerNorm row kernels between the GEMMs (csrc/vit.hip), bit for bit.
tests/golden/row_kernel_hashes.json holds SHA-256 digests of the buffers these kernels write, recorded on an MI355X from the
commit the file names, BEFORE the kernels moved onto the shared row body (csrc/ln_row.h).  Everything goes through entry
points of the product library:

  ln.<rows>x<W>      wise_layernorm_f32_bf16, eps 1e-5: layernorm_narrow_kernel (W <= 128), layernorm_kernel<NV> (one row per
                     wave) and layernorm_rows_kernel<NV, 4> (nv <= 2 and rows >= 16384), both sides of each switch
  vit.*              a shallow image tower (image 16, patch 8: T = 5, K = 192), batch 3: embed_lnpre_kernel<NV> and
                     cls_ln_kernel<NV> without positions, NV 3 and 5; width 768 also with one folded block (the hi + lo and
                     rstd_out branch of embed_lnpre_kernel)
  text.pool<p>       a layers = 0 text tower, width 128: cls_ln_kernel<1> with positions (pooled row first, last, in the middle)
  xlmr               a layers = 0 XLM-R tower, width 256: layernorm_kernel<1> with the fp32 copy xo (right-padded rows)

Inputs come from seeded CPU generators.  Every LayerNorm case carries one constant row (variance 0: rstd = rsqrt(eps)) and
one row with a single 1e4 outlier; the text and XLM-R towers get theirs through two rows of the token embedding (constant up
to the rounding of `c - pos + pos`); the image tower's rows come out of its patch GEMM and have neither.  Every buffer the
test hands to the library has 4 guard rows behind it, prefilled with the bf16 pattern 0x7FC1 (fp32 0x7FC00001), and the digest
covers all of it: a store past `rows` or past W shows.

Recording (on the GPU, from the commit to pin):  python tests/test_gpu_row_kernel_hashes.py <commit> [<output.json>]"""
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

import pytest
import torch

GOLDEN = Path(__file__).resolve().parent / "golden" / "row_kernel_hashes.json"
GUARD = 4
LN_SHAPES = [(5, 96), (9, 96), (3, 128), (2, 4),                                        # half a wave per row
             (7, 132), (3, 256), (5, 260), (7, 768), (5, 1280), (3, 4096),              # one row per wave, nv 1 .. 16
             (16384, 192), (16387, 384), (16383, 192)]                                  # four rows per wave, and just under it
VIT_CASES = [(768, 12, 0, 0), (768, 12, 1, 1), (1280, 16, 0, 0)]                        # width, heads, layers, ln_fold
CASES = [f"ln.{r}x{w}" for r, w in LN_SHAPES] + [f"vit.w{w}.l{l}.fold{f}" for w, _, l, f in VIT_CASES] + \
        ["text.pool0", "text.pool1", "xlmr"]


def _guarded(rows: int, cols: int, dtype) -> torch.Tensor:
    """[rows + GUARD, cols] on the device, every element the quiet-NaN pattern no kernel here produces"""
    t = torch.empty(rows + GUARD, cols, dtype=dtype, device="cuda")
    if dtype == torch.bfloat16:
        t.view(torch.int16).fill_(0x7FC1)
    else:
        t.view(torch.int32).fill_(0x7FC00001)
    return t


def _digest(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        a = t.detach().cpu().contiguous()
        a = a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32)
        h.update(f"{t.dtype}{tuple(t.shape)}".encode())
        h.update(a.numpy().tobytes())
    return h.hexdigest()


def _ln_case(rows: int, W: int) -> dict:
    from wise_amd import _lib
    lib = _lib.lib()
    g = torch.Generator().manual_seed(rows * 8192 + W)
    x = torch.randn(rows, W, generator=g) * 3 + 0.5
    w = 1 + 0.1 * torch.randn(W, generator=g)
    b = 0.1 * torch.randn(W, generator=g)
    x[rows - 1, :] = 1.25                  # variance 0
    x[rows - 2, W // 3] = 1e4              # one outlier
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    y = _guarded(rows, W, torch.bfloat16)
    _lib.check(lib.wise_layernorm_f32_bf16(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), rows, W, 1e-5, y.data_ptr(),
                                           _lib.stream_ptr()), "wise_layernorm_f32_bf16")
    torch.cuda.synchronize()
    return {"y": _digest(y)}


def _vit_case(width: int, heads: int, layers: int, fold: int) -> dict:
    from wise_amd import _lib
    from wise_amd.feature.vit import VitEngine, VitSpec, random_state_dict
    B = 3       # 15 rows: the last block of four waves is ragged
    spec = VitSpec("rows", 16, 8, width, layers, heads, 4 * width, 64)
    eng = VitEngine(spec, random_state_dict(spec, 5), max_batch=B, ln_fold=fold)
    assert eng.spec.ln_fold == fold
    frames = torch.randint(0, 256, (B, 3, 16, 16), generator=torch.Generator().manual_seed(width + layers), dtype=torch.uint8)
    x, kind = eng._check_images(frames)
    out = {}
    for name, single in (("single", True), ("halves", False)):
        o = _guarded(B, spec.embed_dim, torch.float32)
        _lib.check(eng._call(kind, single, x, o, eng._ws, _lib.stream_ptr()), "wise_vit_forward")
        res = _guarded(B * spec.tokens, width, torch.float32)
        _lib.check(eng.lib.wise_vit_tap_residual(C.byref(eng.cfg), B, eng._ws.data_ptr(), res.data_ptr(), _lib.stream_ptr()),
                   "wise_vit_tap_residual")
        torch.cuda.synchronize()
        out[f"{name}.out"] = _digest(o)
        out[f"{name}.residual"] = _digest(res)
    return out


def _text_case(pool: str) -> dict:
    from wise_amd.feature.text import TextEngine, TextSpec, random_text_state_dict
    T, V = 8, 32
    spec = TextSpec("rows", 128, 2, 0, 64, context=T, vocab=V, pool=pool)
    sd = random_text_state_dict(spec, 3)
    # id 31 is the largest (argmax pooling); 0 is the pad id of last_nonzero pooling.  Pooled position: first, last, middle,
    # then a constant row (id 30 at position 2) and an outlier row (id 29)
    if pool == "argmax":
        tok = torch.tensor([[31, 4, 5, 6, 7, 8, 9, 10], [4, 5, 6, 7, 8, 9, 10, 31], [4, 5, 6, 31, 7, 8, 31, 9],
                            [4, 5, 30, 6, 7, 8, 9, 10], [4, 5, 6, 7, 29, 8, 9, 10]], dtype=torch.int32)
    else:
        tok = torch.tensor([[31, 0, 0, 0, 0, 0, 0, 0], [4, 5, 6, 7, 8, 9, 10, 31], [4, 5, 6, 31, 0, 0, 0, 0],
                            [4, 5, 30, 0, 0, 0, 0, 0], [4, 5, 6, 7, 29, 0, 0, 0]], dtype=torch.int32)
    sd["token_embedding.weight"][30] = 0.75 - sd["positional_embedding"][2]
    sd["token_embedding.weight"][29, 41] = 1e4
    eng = TextEngine(spec, sd, max_batch=tok.shape[0])
    out = _guarded(tok.shape[0], spec.embed_dim, torch.float32)
    eng._launch(tok.cuda(), out)
    torch.cuda.synchronize()
    return {"out": _digest(out)}


def _xlmr_case() -> dict:
    from wise_amd import _lib
    from wise_amd.feature.xlmr_text import XlmrSpec, XlmrTextEngine, random_xlmr_state_dict
    T, V, PAD = 8, 32, 1
    spec = XlmrSpec("rows", 256, 4, 0, 1024, 64, vocab=V, max_positions=T + PAD + 1, context=T, pad_id=PAD)
    sd = random_xlmr_state_dict(spec, 3)
    e = "text.transformer.embeddings."
    # id 30 at position 2 (position row 2 + 1 + PAD = 4 of RoBERTa's cumsum): a constant row; id 29: an outlier
    sd[e + "word_embeddings.weight"][30] = 0.75 - sd[e + "position_embeddings.weight"][4] - sd[e + "token_type_embeddings.weight"][0]
    sd[e + "word_embeddings.weight"][29, 77] = 1e4
    lens = [8, 1, 5, 3, 6, 2, 7]            # 56 rows: 14 blocks of four waves
    tok = torch.full((len(lens), T), PAD, dtype=torch.int32)
    for r, n in enumerate(lens):
        tok[r, :n] = torch.arange(n, dtype=torch.int32) + 4 + r
    tok[0, 2], tok[2, 3] = 30, 29
    eng = XlmrTextEngine(spec, sd, max_batch=tok.shape[0])
    out = _guarded(tok.shape[0], spec.embed_dim, torch.float32)
    eng._launch(tok.cuda(), out)
    res = _guarded(tok.shape[0] * T, spec.width, torch.float32)
    _lib.check(eng.lib.wise_xlmr_tap_residual(C.byref(eng.cfg), tok.shape[0], eng._ws.data_ptr(), res.data_ptr(),
                                              _lib.stream_ptr()), "wise_xlmr_tap_residual")
    torch.cuda.synchronize()
    return {"out": _digest(out), "residual": _digest(res)}


def surface(case: str) -> dict:
    kind, _, rest = case.partition(".")
    if kind == "ln":
        rows, W = rest.split("x")
        return _ln_case(int(rows), int(W))
    if kind == "vit":
        return _vit_case(*next(c for c in VIT_CASES if case == f"vit.w{c[0]}.l{c[2]}.fold{c[3]}"))
    if kind == "text":
        return _text_case({"pool0": "argmax", "pool1": "last_nonzero"}[rest])
    return _xlmr_case()


def record(commit: str, path: Path = GOLDEN) -> None:
    """Write the golden file: run on the GPU from the commit whose behaviour is to be pinned."""
    path.write_text(json.dumps({"commit": commit, "hashes": {case: surface(case) for case in CASES}}, indent=1) + "\n")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_rows_equal_the_recorded_digests(case):
    want = json.loads(GOLDEN.read_text())["hashes"][case]
    got = surface(case)
    assert sorted(got) == sorted(want)
    assert got == want, sorted(key for key in want if got[key] != want[key])


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    record(sys.argv[1], Path(sys.argv[2]) if len(sys.argv) > 2 else GOLDEN)

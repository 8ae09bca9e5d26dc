"""The tile plan of the bf16 GEMM family (csrc/gemm_bf16.hip: gemm_plan, fold_plan, conv_plan) on every GEMM shape the
towers issue, against the table in tests/golden/gemm_plan.txt.  The plan is host code and launches nothing, so the debug
library answers without a GPU (wise_debug_gemm_plan).  A changed row means some shape now runs another tile.

    python tests/test_gemm_plan_cpu.py > tests/golden/gemm_plan.txt   # rewrites the table (only for a policy change)"""
import ctypes as C
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
LIB_DEBUG = ROOT / "wise_amd" / "lib" / "libwise_hip_debug.so"
GOLDEN = ROOT / "tests" / "golden" / "gemm_plan.txt"

# epilogue modes (csrc/gemm_shared.h)
BF16, QUICKGELU, GELU, GELU_TANH, RESID, F32, RELU = 0, 1, 2, 5, 3, 4, 6
BATCHES = (1, 37, 128, 256, 512)
CUS = 256


def _pad(m, to):
    return (m + to - 1) // to * to


def _vit(name, W, F, T, act, patch_k, D, fold=True, head=None):
    """(label, M, N, K, mode, m_valid) of a ViT-style image tower per batch: patch embedding, the four block GEMMs,
    the projection head; fold: the same block GEMMs in the LayerNorm-fold form"""
    Kp = _pad(patch_k, 64)
    for b in BATCHES:
        Mp, Mpp, Bp = _pad(b * T, 256), _pad(b * (T - 1), 256), _pad(b, 256)
        yield "gemm", f"{name} bs={b} patch", (Mpp, W, Kp, F32, 0)
        yield "gemm", f"{name} bs={b} qkv", (Mp, 3 * W, W, BF16, Mp)
        yield "gemm", f"{name} bs={b} out", (Mp, W, W, RESID, Mp)
        yield "gemm", f"{name} bs={b} fc1", (Mp, F, W, act, Mp)
        yield "gemm", f"{name} bs={b} fc2", (Mp, W, F, RESID, Mp)
        yield "gemm", f"{name} bs={b} proj", (Bp, D, W, F32, 0)
        if head:
            for lab, sh in head(b):
                yield "gemm", f"{name} bs={b} {lab}", sh
        if fold:
            yield "fold", f"{name} bs={b} qkv", (Mp, 3 * W, W, BF16, 0, 0)
            yield "fold", f"{name} bs={b} out", (Mp, W, W, RESID, 1, 0)
            yield "fold", f"{name} bs={b} fc1", (Mp, F, W, act, 0, 0)
            yield "fold", f"{name} bs={b} fc2", (Mp, W, F, RESID, 1, 0)
        # half batches (two halves in flight) run at their own row counts
        if b >= 128:
            h = b // 2
            Mh = _pad(h * T, 256)
            yield "gemm", f"{name} half={h} qkv", (Mh, 3 * W, W, BF16, Mh)
            yield "gemm", f"{name} half={h} fc1", (Mh, F, W, act, Mh)
            yield "gemm", f"{name} half={h} fc2", (Mh, W, F, RESID, Mh)


def _siglip_head(W, F):
    def head(b):
        Bp = _pad(b, 256)
        Mp = _pad(b * 576, 256)
        yield "head kv", (Mp, 2 * W, W, BF16, 0)
        yield "head proj", (Bp, W, W, F32, 0)
        yield "head fc1", (Bp, F, W, GELU, 0)
        yield "head fc2", (Bp, W, F, RESID, 0)
    return head


def _text(name, W, F, D, act, lengths):
    """text towers: one query (skinny: split-K where it applies) up to 256 queries"""
    for q in (1, 2, 37, 256):
        for T in lengths:
            M = q * T
            Mp = _pad(M, 256)
            Mv = M if M <= 128 else Mp
            yield "gemm", f"{name} q={q} T={T} qkv", (Mp, 3 * W, W, BF16, Mv)
            yield "gemm", f"{name} q={q} T={T} out", (Mp, W, W, RESID, Mv)
            yield "gemm", f"{name} q={q} T={T} fc1", (Mp, F, W, act, Mv)
            yield "gemm", f"{name} q={q} T={T} fc2", (Mp, W, F, RESID, Mv)
        Bp = _pad(q, 256)
        yield "gemm", f"{name} q={q} proj", (Bp, D, W, F32, q)


def _htsat():
    """MS-CLAP HTSAT: four Swin stages (C = 96 .. 768, 4096 / 1024 / 256 / 64 tokens a clip), the patch merges, the head"""
    for b in (1, 7, 64, 128, 256):
        for C_, tok in ((96, 4096), (192, 1024), (384, 256), (768, 64)):
            Mp = _pad(b * tok, 128)
            yield "gemm", f"htsat bs={b} C={C_} qkv", (Mp, 3 * C_, C_, BF16, 0)
            yield "gemm", f"htsat bs={b} C={C_} proj", (Mp, C_, C_, RESID, 0)
            yield "gemm", f"htsat bs={b} C={C_} fc1", (Mp, 4 * C_, C_, GELU, 0)
            yield "gemm", f"htsat bs={b} C={C_} fc2", (Mp, C_, 4 * C_, RESID, 0)
            if C_ < 768:
                M2p = _pad(b * tok // 4, 128)
                yield "gemm", f"htsat bs={b} C={C_} merge", (M2p, 2 * C_, 4 * C_, F32, 0)
                yield "fold", f"htsat bs={b} C={C_} merge", (M2p, 2 * C_, 4 * C_, F32, 1, 1)
            yield "fold", f"htsat bs={b} C={C_} qkv", (Mp, 3 * C_, C_, BF16, 0, 1)
            yield "fold", f"htsat bs={b} C={C_} proj", (Mp, C_, C_, RESID, 1, 1)
            yield "fold", f"htsat bs={b} C={C_} fc1", (Mp, 4 * C_, C_, GELU, 0, 1)
            yield "fold", f"htsat bs={b} C={C_} fc2", (Mp, C_, 4 * C_, RESID, 1, 1)
        Bp = _pad(b, 128)
        yield "gemm", f"htsat bs={b} head e", (Bp, 1024, 768, F32, 0)
        yield "gemm", f"htsat bs={b} head g", (Bp, 1024, 768, GELU, 0)
        yield "gemm", f"htsat bs={b} head out", (Bp, 1024, 1024, RESID, 0)


def _cnn14():
    """PANNs Cnn14 (10 s clips: 1001 frames x 64 mel bins): the ten 3x3 convolutions after the first, and fc1"""
    for b in (1, 7, 64, 128):
        T, F = 1001, 64
        chans = (64, 128, 256, 512, 1024, 2048)
        for i, cout in enumerate(chans):
            cin = 1 if i == 0 else chans[i - 1]
            if i > 0:
                yield "conv", f"cnn14 bs={b} block{i + 1} conv1", (b, T, F, cin, cout, 0)
            yield "conv", f"cnn14 bs={b} block{i + 1} conv2", (b, T, F, cout, cout, 1)
            T, F = T // 2, F // 2
        yield "gemm", f"cnn14 bs={b} fc1", (_pad(b, 128), 2048, 2048, RELU, 0)


def cases():
    yield from _vit("ViT-B/32", 768, 3072, 50, QUICKGELU, 3 * 32 * 32, 512)
    yield from _vit("ViT-B/16", 768, 3072, 197, QUICKGELU, 3 * 16 * 16, 512)
    yield from _vit("ViT-L/14", 1024, 4096, 257, QUICKGELU, 3 * 14 * 14, 768)
    yield from _vit("ViT-H/14", 1280, 5120, 257, GELU, 3 * 14 * 14, 1024)
    yield from _vit("SigLIP-L/16-384", 1024, 4096, 577, GELU_TANH, 3 * 16 * 16, 1024, head=_siglip_head(1024, 4096))
    yield from _text("CLIP-text", 512, 2048, 512, QUICKGELU, (77,))
    yield from _text("CLIP-text-L", 768, 3072, 768, QUICKGELU, (77,))
    yield from _text("GPT2-text", 768, 3072, 1024, GELU_TANH, (77,))
    yield from _text("XLM-R", 1024, 4096, 768, GELU, (8, 24, 77))
    yield from _htsat()
    yield from _cnn14()


def plan_lines(lib):
    out = (C.c_int * 8)()
    lines = []
    for kind, label, args in cases():
        if kind == "gemm":
            for ov in (0, 1):
                a = (C.c_int * 7)(*args, ov, CUS)
                assert lib.wise_debug_gemm_plan(0, a, out) == 6
                splitk, n, v0, r0, v1, r1 = out[:6]
                plan = f"splitk={splitk} " + (f"v={v0}" if n == 1 else f"v={v0} x {r0} rows + v={v1} x {r1} rows")
                lines.append(f"gemm  {label:32s} M={args[0]} N={args[1]} K={args[2]} mode={args[3]} m_valid={args[4]} "
                             f"overlapped={ov} -> {plan}")
        elif kind == "fold":
            a = (C.c_int * 7)(*args, CUS)
            assert lib.wise_debug_gemm_plan(1, a, out) == 1
            lines.append(f"fold  {label:32s} M={args[0]} N={args[1]} K={args[2]} mode={args[3]} producer={args[4]} "
                         f"wide96={args[5]} -> v={out[0]}")
        else:
            a = (C.c_int * 7)(*args, 0)
            assert lib.wise_debug_gemm_plan(2, a, out) == 1
            tile = ("128x64", "128x128", "256x64", "pp256x256")[out[0]]
            lines.append(f"conv  {label:32s} B={args[0]} T={args[1]} F={args[2]} Cin={args[3]} Cout={args[4]} "
                         f"pool={args[5]} -> {tile}")
    return lines


def _load():
    if not LIB_DEBUG.exists():
        pytest.skip("libwise_hip_debug.so not built (python -m wise_amd.build)")
    lib = C.CDLL(str(LIB_DEBUG))
    lib.wise_debug_gemm_plan.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.wise_debug_gemm_plan.restype = C.c_int
    return lib


def test_gemm_plan_matches_table():
    got = plan_lines(_load())
    want = GOLDEN.read_text().splitlines()
    assert len(got) == len(want), f"{len(got)} plan rows, the table has {len(want)}"
    moved = [f"  table: {w}\n  now:   {g}" for w, g in zip(want, got) if w != g]
    assert not moved, f"{len(moved)} shapes plan another tile:\n" + "\n".join(moved[:20])


def test_splitk_scratch_bytes_follow_the_plan():
    """Every row of the table with m_valid > 0 (gemm_bf16_rows): the scratch a call asks for is the plan's S partial tiles
    of 128 rows, fp32 — 0 where the plan does not split."""
    lib = _load()
    lib.wise_debug_gemm_splitk_bytes.argtypes = [C.c_int] * 4
    lib.wise_debug_gemm_splitk_bytes.restype = C.c_size_t
    out = (C.c_int * 8)()
    rows = split = 0
    for kind, label, args in cases():
        if kind != "gemm" or args[4] <= 0:
            continue
        M, N, K, mode, m_valid = args
        for ov in (0, 1):
            assert lib.wise_debug_gemm_plan(0, (C.c_int * 7)(*args, ov, CUS), out) == 6
            assert lib.wise_debug_gemm_splitk_bytes(M, m_valid, N, K) == out[0] * 128 * N * 4, label
        rows += 1
        split += out[0] > 0
    assert rows and 0 < split < rows      # the table has both kinds


if __name__ == "__main__":
    lib = C.CDLL(str(LIB_DEBUG))
    lib.wise_debug_gemm_plan.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    sys.stdout.write("\n".join(plan_lines(lib)) + "\n")

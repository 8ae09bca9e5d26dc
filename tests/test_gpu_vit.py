"""-m gpu: HP-1 parity — HIP ViT kernels (through the C ABI) against the fp32 CPU oracle and the
committed golden vectors.  Tolerance (BASELINE.json north_star): cosine within 1e-3 of the fp32 path."""
import numpy as np
import pytest
import torch

from oracle import vit_ref
from wise_amd import _lib
from wise_amd.feature.vit import checkpoint_like_state_dict, VitEngine, VitSpec, random_state_dict, spec_for

pytestmark = pytest.mark.gpu

COS_TOL = 1e-3


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def cosine(a, b):
    a = a.double(); b = b.double()
    return ((a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))).min().item()


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 384, 192), (12800, 768, 768), (1280, 2304, 768),
                                    (640, 768, 3072), (12544, 768, 3072),
                                    # 256x256 ping-pong (225 tiles) and 320x256 ping-pong (240 tiles) tilings
                                    (6400, 2304, 768), (6400, 3072, 768),
                                    # 256x192 / 128x192 / 128x256 tiles (HTSAT stages 2-4: power-of-two rows, short K)
                                    (32768, 384, 384), (8192, 768, 3072), (16384, 576, 192), (8192, 1536, 384),
                                    # ... and the two-workgroups-per-CU tiles for short K: 128x192 (above) and 128x128
                                    (32768, 256, 192),
                                    # HTSAT shapes: N edge (N % 128 != 0) and K % 64 != 0
                                    (256, 288, 96), (128, 96, 384), (384, 192, 96), (256, 576, 192), (128, 36, 32)])
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4, 5, 6])
def test_gemm_modes(M, N, K, mode):
    if M > 2000 and mode not in (0, 3, 5, 6) and (M, N, K) != (8192, 1536, 384):
        pytest.skip("large shapes: bf16-out, residual, tanh-GELU and ReLU modes only")
    lib = _lib.lib()
    g = torch.Generator().manual_seed(M + N + K + mode)
    A = bf16_round(torch.randn(M, K, generator=g))
    W = bf16_round(torch.randn(N, K, generator=g) * K ** -0.5)
    bias = torch.randn(N, generator=g)
    ref = A.double() @ W.double().t() + bias.double()
    Ad, Wd, bd = A.to(torch.bfloat16).cuda(), W.to(torch.bfloat16).cuda(), bias.cuda()
    if mode == 3:
        resid = torch.randn(M, N, generator=g)
        out = resid.clone().cuda()
        ref = ref + resid.double()
    elif mode == 4:
        out = torch.empty(M, N, dtype=torch.float32, device="cuda")
    else:
        out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        if mode == 1:
            ref = ref * torch.sigmoid(1.702 * ref)
        elif mode == 2:
            ref = 0.5 * ref * (1 + torch.erf(ref / 2 ** 0.5))
        elif mode == 5:
            ref = 0.5 * ref * (1 + torch.tanh(0.7978845608028654 * (ref + 0.044715 * ref ** 3)))
        elif mode == 6:
            ref = ref.clamp(min=0)
    _lib.check(lib.wise_gemm_bf16(Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), M, N, K, mode, out.data_ptr(),
                                  _lib.stream_ptr()), "gemm")
    torch.cuda.synchronize()
    got = out.float().cpu().double()
    err = (got - ref).abs().max().item()
    tol = 2e-3 if mode in (3, 4) else 3e-2  # fp32 out: accumulation order only; bf16 out: one bf16 rounding of O(4) values
    assert err <= tol, (err, tol)
    if mode in (3, 4):
        assert torch.allclose(got, ref, atol=2e-3, rtol=1e-5)


def test_gemm_identity_asymmetric():
    """A = I (padded) against an asymmetric W: catches a transposed C-write or a bad swizzle."""
    lib = _lib.lib()
    M = N = 128; K = 128
    A = torch.eye(M, K)
    W = (torch.arange(N * K, dtype=torch.float32).reshape(N, K) % 251) - 125  # exact in bf16 (|v| <= 125)
    out = torch.empty(M, N, dtype=torch.float32, device="cuda")
    Ad, Wd = A.to(torch.bfloat16).cuda(), W.to(torch.bfloat16).cuda()  # keep alive across the launch
    _lib.check(lib.wise_gemm_bf16(Ad.data_ptr(), Wd.data_ptr(), 0, M, N, K, 4, out.data_ptr(), _lib.stream_ptr()),
               "gemm")
    assert torch.equal(out.cpu(), W.t().contiguous()[:M, :N])


@pytest.mark.parametrize("rows,W", [(1, 768), (50, 768), (12800, 768), (257, 1024), (5, 96), (7, 3072), (3, 4096)])
def test_layernorm(rows, W):
    lib = _lib.lib()
    g = torch.Generator().manual_seed(rows + W)
    x = torch.randn(rows, W, generator=g) * 3 + 0.5
    w = 1 + 0.1 * torch.randn(W, generator=g)
    b = 0.1 * torch.randn(W, generator=g)
    y = torch.empty(rows, W, dtype=torch.bfloat16, device="cuda")
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()  # keep alive across the launch
    _lib.check(lib.wise_layernorm_f32_bf16(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), rows, W, 1e-5, y.data_ptr(),
                                           _lib.stream_ptr()), "ln")
    ref = vit_ref.layer_norm(x, w, b)
    # at most 1 bf16 ulp from the fp32 oracle rounded to bf16
    assert (y.float().cpu() - bf16_round(ref)).abs().max() <= 2 ** -7 * ref.abs().max()


@pytest.mark.parametrize("B,T,H", [(1, 1, 2), (3, 50, 12), (2, 257, 16), (2, 64, 2), (1, 65, 2), (5, 197, 12)])
def test_attention(B, T, H):
    lib = _lib.lib()
    g = torch.Generator().manual_seed(B * 1000 + T + H)
    W = H * 64
    qkv = torch.randn(B * T, 3 * W, generator=g)
    qkv[:, : 2 * W] *= 2.0  # peaky softmax
    qkv = bf16_round(qkv)
    o = torch.full((B * T, W), float("nan"), dtype=torch.bfloat16, device="cuda")
    qd = qkv.to(torch.bfloat16).cuda()  # keep alive across the launch
    _lib.check(lib.wise_attention_bf16(qd.data_ptr(), B, T, H, o.data_ptr(), _lib.stream_ptr()), "attn")
    ref = vit_ref.attention_ref(qkv, B, T, H)
    got = o.float().cpu()
    assert torch.isfinite(got).all()
    assert (got - ref).abs().max().item() <= 3e-2
    assert cosine(got, ref) >= 1 - 1e-4


@pytest.mark.parametrize("B,T,H", [(1, 1, 8), (2, 26, 8), (2, 82, 8), (1, 64, 16), (3, 257, 16), (1, 300, 8)])
def test_attention_head_dim_80(B, T, H):
    """ViT-H/14's head width: three 32-deep steps of QK^T with the tail zero, five 16-channel tiles of PV"""
    lib = _lib.lib()
    g = torch.Generator().manual_seed(B * 1000 + T + H)
    W = H * 80
    qkv = torch.randn(B * T, 3 * W, generator=g)
    qkv[:, : 2 * W] *= 1.8
    qkv = bf16_round(qkv)
    o = torch.full((B * T, W), float("nan"), dtype=torch.bfloat16, device="cuda")
    qd = qkv.to(torch.bfloat16).cuda()
    _lib.check(lib.wise_attention_dh_bf16(qd.data_ptr(), B, T, H, 80, o.data_ptr(), _lib.stream_ptr()), "attn")
    ref = vit_ref.attention_ref(qkv, B, T, H, 80)
    got = o.float().cpu()
    assert torch.isfinite(got).all()
    assert (got - ref).abs().max().item() <= 3e-2
    assert cosine(got, ref) >= 1 - 1e-4
    # head dim 64 through the same entry equals the plain one
    qkv64 = bf16_round(torch.randn(B * T, 3 * H * 64, generator=g)).to(torch.bfloat16).cuda()
    o1 = torch.empty(B * T, H * 64, dtype=torch.bfloat16, device="cuda"); o2 = torch.empty_like(o1)
    _lib.check(lib.wise_attention_dh_bf16(qkv64.data_ptr(), B, T, H, 64, o1.data_ptr(), _lib.stream_ptr()), "attn")
    _lib.check(lib.wise_attention_bf16(qkv64.data_ptr(), B, T, H, o2.data_ptr(), _lib.stream_ptr()), "attn")
    assert torch.equal(o1, o2)
    assert lib.wise_attention_dh_bf16(qkv64.data_ptr(), B, T, H, 72, o1.data_ptr(), _lib.stream_ptr()) != 0


def load_golden(golden_dir, name):
    g = np.load(golden_dir / name)
    s = [int(v) for v in g["spec"]]
    spec = VitSpec(name, s[0], s[1], s[2], s[3], s[4], s[5], s[6], "quick_gelu" if s[7] == 0 else "gelu")
    frames = np.random.default_rng(int(g["frame_seed"])).integers(0, 256, size=(int(g["n_frames"]), 3, s[0], s[0]),
                                                                  dtype=np.uint8)
    return spec, g, torch.from_numpy(frames)


@pytest.mark.parametrize("name", ["vit_tiny.npz", "vit_tiny_gelu.npz", "vit_tiny_h80.npz", "vit_b32.npz", "vit_b16.npz",
                                  "vit_l14.npz", "vit_h14.npz"])
def test_vit_golden(golden_dir, name):
    spec, g, frames = load_golden(golden_dir, name)
    sd = random_state_dict(spec, int(g["weight_seed"]))
    eng = VitEngine(spec, sd, max_batch=frames.shape[0])
    out_u8 = eng.forward(frames).cpu()
    out_f32 = eng.forward(vit_ref.normalize_u8(frames)).cpu()
    gold = torch.from_numpy(g["out"])
    assert out_u8.shape == gold.shape and out_u8.dtype == torch.float32
    assert torch.allclose(out_u8.norm(dim=1), torch.ones(gold.shape[0]), atol=1e-5)
    c = cosine(out_f32, gold)
    assert c >= 1 - COS_TOL, c
    assert cosine(out_u8, gold) >= 1 - COS_TOL
    # residual stream after the last block: compare the cls rows with the oracle's last tap
    taps = torch.from_numpy(g["taps"])
    x = eng.residual(frames.shape[0]).cpu().reshape(frames.shape[0], spec.tokens, spec.width)
    last = taps[-1] if taps.dim() == 3 else taps[-1][:, 0, :]
    assert cosine(x[:, 0, :], last) >= 1 - COS_TOL
    if taps.dim() == 4:  # tiny models carry every token
        assert cosine(x.reshape(-1, spec.width), taps[-1].reshape(-1, spec.width)) >= 1 - COS_TOL


@pytest.mark.parametrize("name", ["vit_tiny_stress.npz", "vit_b32_stress.npz", "vit_l14_stress.npz"])
def test_vit_checkpoint_like_golden(golden_dir, name):
    """Parity on weights with the statistics of real checkpoints (wise_amd/feature/vit.py::checkpoint_like_state_dict:
    massive-activation channels at 40-100x the typical magnitude, log-normal LayerNorm gains, 3x embeddings, near one-hot
    attention rows) — what the benign Gaussian fixtures do not exercise.  The oracle was pinned to transformers' CLIP on
    these same weights (oracle/make_golden.py); the bf16 HIP path must keep the fp32 contract of
    src/feature/mlfoundation_openclip.py:99-100 to cosine >= 1 - 1e-3, and the residual stream of the last block too."""
    spec, g, frames = load_golden(golden_dir, name)
    sd = checkpoint_like_state_dict(spec, int(g["weight_seed"]))
    eng = VitEngine(spec, sd, max_batch=frames.shape[0])
    out = eng.forward(vit_ref.normalize_u8(frames)).cpu()
    gold = torch.from_numpy(g["out"])
    c = cosine(out, gold)
    assert c >= 1 - COS_TOL, c
    assert cosine(eng.forward(frames).cpu(), gold) >= 1 - COS_TOL
    taps = torch.from_numpy(g["taps"])
    x = eng.residual(frames.shape[0]).cpu().reshape(frames.shape[0], spec.tokens, spec.width)
    last = taps[-1] if taps.dim() == 3 else taps[-1][:, 0, :]
    assert cosine(x[:, 0, :], last) >= 1 - COS_TOL
    assert float(last.abs().max()) >= 40.0            # the fixture does carry massive activations


@pytest.mark.parametrize("layers", [0, 1, 3])
def test_vit_b32_depth_taps(golden_dir, layers):
    """Truncated ViT-B/32 against the per-block golden taps: localises an error to a block."""
    spec, g, frames = load_golden(golden_dir, "vit_b32.npz")
    sd = random_state_dict(spec, int(g["weight_seed"]))
    short = VitSpec(spec.name, spec.image_size, spec.patch, spec.width, layers, spec.heads, spec.mlp, spec.embed_dim,
                    spec.act)
    sd_short = {k: v for k, v in sd.items()
                if "resblocks." not in k or int(k.split("resblocks.")[1].split(".")[0]) < layers}
    eng = VitEngine(short, sd_short, max_batch=4)
    eng.forward(vit_ref.normalize_u8(frames))
    x = eng.residual(4).cpu().reshape(4, spec.tokens, spec.width)
    tap = torch.from_numpy(g["taps"])[layers]
    assert cosine(x[:, 0, :], tap) >= 1 - 2e-4
    assert (x[:, 0, :] - tap).abs().max() <= 0.05 * tap.abs().max()


def test_vit_b32_batch256_consistency(golden_dir):
    """BASELINE cfg-2 shape: bs=256.  Frames 0..3 are the golden frames; every row must be unit-norm,
    the golden rows must match, and the result must not depend on the batch a frame sits in."""
    spec, g, frames = load_golden(golden_dir, "vit_b32.npz")
    sd = random_state_dict(spec, int(g["weight_seed"]))
    eng = VitEngine(spec, sd, max_batch=256)
    rest = torch.from_numpy(np.random.default_rng(99).integers(0, 256, size=(252, 3, 224, 224), dtype=np.uint8))
    batch = torch.cat([frames, rest], dim=0)
    out = eng.forward(batch).cpu()
    assert out.shape == (256, 512)
    assert torch.allclose(out.norm(dim=1), torch.ones(256), atol=1e-5)
    assert cosine(out[:4], torch.from_numpy(g["out"])) >= 1 - COS_TOL
    perm = torch.randperm(256, generator=torch.Generator().manual_seed(0))
    out_p = eng.forward(batch[perm]).cpu()
    assert torch.equal(out_p, out[perm])  # deterministic kernels, frames independent
    # ragged batch (not a multiple of anything)
    out_r = eng.forward(batch[:37]).cpu()
    assert torch.equal(out_r, out[:37])


def test_vit_l14_batch256_consistency(golden_dir):
    """BASELINE cfg-4, image half: ViT-L/14 at bs=256 (the reference's own shape test: [8,768] from ViT-L-14,
    src/feature/test_feature_extractor.py:33-34).  Frames 0..1 are the golden frames; every row unit-norm, golden rows
    match the oracle's vectors, results independent of the batch a frame sits in, pipelined == one at a time."""
    spec, g, frames = load_golden(golden_dir, "vit_l14.npz")
    sd = random_state_dict(spec, int(g["weight_seed"]))
    eng = VitEngine(spec, sd, max_batch=256)
    n_gold = frames.shape[0]
    rest = torch.from_numpy(np.random.default_rng(98).integers(0, 256, size=(256 - n_gold, 3, 224, 224), dtype=np.uint8))
    batch = torch.cat([frames, rest], dim=0)
    out = eng.forward(batch).cpu()
    assert out.shape == (256, 768) and out.dtype == torch.float32
    assert torch.allclose(out.norm(dim=1), torch.ones(256), atol=1e-5)
    assert cosine(out[:n_gold], torch.from_numpy(g["out"])) >= 1 - COS_TOL
    perm = torch.randperm(256, generator=torch.Generator().manual_seed(1))
    assert torch.equal(eng.forward(batch[perm]).cpu(), out[perm])
    assert torch.equal(eng.forward(batch, single_stream=True).cpu(), out)
    assert torch.equal(eng.forward_pipelined(batch).result().cpu(), out)
    assert torch.equal(eng.forward(batch[:19]).cpu(), out[:19])


@pytest.mark.parametrize("M,N,K,mode", [(256, 288, 96, 0), (1024, 384, 96, 2), (128, 576, 192, 0), (256, 768, 192, 2),
                                        (128, 96, 96, 0), (384, 200, 96, 1), (128, 1024, 192, 5)])
def test_gemm_with_fused_layernorm(M, N, K, mode):
    """wise_gemm_ln_bf16 (HTSAT stages 1-2): LayerNorm computed inside the GEMM's A-tile build."""
    lib = _lib.lib()
    g = torch.Generator().manual_seed(M + N + K + mode)
    x = torch.randn(M, K, generator=g) * 2 + 0.3
    lw = 1 + 0.1 * torch.randn(K, generator=g)
    lb = 0.1 * torch.randn(K, generator=g)
    W = bf16_round(torch.randn(N, K, generator=g) * K ** -0.5)
    bias = torch.randn(N, generator=g)
    h = bf16_round(torch.nn.functional.layer_norm(x, (K,), lw, lb, 1e-5))
    ref = h.double() @ W.double().t() + bias.double()
    if mode == 1:
        ref = ref * torch.sigmoid(1.702 * ref)
    elif mode == 2:
        ref = 0.5 * ref * (1 + torch.erf(ref / 2 ** 0.5))
    elif mode == 5:
        ref = 0.5 * ref * (1 + torch.tanh(0.7978845608028654 * (ref + 0.044715 * ref ** 3)))
    xd, lwd, lbd, Wd, bd = x.cuda(), lw.cuda(), lb.cuda(), W.to(torch.bfloat16).cuda(), bias.cuda()
    out = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.wise_gemm_ln_bf16(xd.data_ptr(), lwd.data_ptr(), lbd.data_ptr(), Wd.data_ptr(), bd.data_ptr(), M, N, K,
                                     1e-5, mode, out.data_ptr(), _lib.stream_ptr()), "gemm_ln")
    torch.cuda.synchronize()
    err = (out.float().cpu().double() - ref).abs().max().item()
    assert err <= 4e-2, err   # one bf16 rounding of the normalised activations and one of O(4) outputs


@pytest.mark.parametrize("M", [128, 1024, 4096])
def test_fused_mlp96(M):
    """wise_mlp96_fused (HTSAT stage 1): x += fc2(gelu(fc1(LN(x)))) with the hidden layer kept on chip."""
    lib = _lib.lib()
    g = torch.Generator().manual_seed(M)
    C, HID = 96, 384
    x = torch.randn(M, C, generator=g) * 1.5 + 0.2
    lw = 1 + 0.1 * torch.randn(C, generator=g)
    lb = 0.1 * torch.randn(C, generator=g)
    W1 = bf16_round(torch.randn(HID, C, generator=g) * C ** -0.5)
    b1 = 0.1 * torch.randn(HID, generator=g)
    W2 = bf16_round(torch.randn(C, HID, generator=g) * HID ** -0.5)
    b2 = 0.1 * torch.randn(C, generator=g)
    h = bf16_round(torch.nn.functional.layer_norm(x, (C,), lw, lb, 1e-5)).double()
    hid = h @ W1.double().t() + b1.double()
    hid = bf16_round((0.5 * hid * (1 + torch.erf(hid / 2 ** 0.5))).float()).double()
    ref = x.double() + hid @ W2.double().t() + b2.double()
    xd = x.clone().cuda()
    keep = [t.cuda() for t in (lw, lb, W1.to(torch.bfloat16), b1, W2.to(torch.bfloat16), b2)]
    _lib.check(lib.wise_mlp96_fused(xd.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(),
                                    keep[3].data_ptr(), keep[4].data_ptr(), keep[5].data_ptr(), M, 1e-5,
                                    _lib.stream_ptr()), "mlp96")
    torch.cuda.synchronize()
    err = (xd.cpu().double() - ref).abs().max().item()
    assert err <= 2e-2, err


def test_pipelined_batches_equal_one_at_a_time():
    """VitEngine.forward_pipelined (two batches in flight, each on its own stream and workspace) must return exactly
    what forward() returns, for every batch, whatever order the results are collected in."""
    spec = spec_for("ViT-B-32", "openai")
    eng = VitEngine(spec, random_state_dict(spec, 0), max_batch=96)
    g = torch.Generator().manual_seed(5)
    batches = [torch.randn(n, 3, 224, 224, generator=g).cuda() for n in (96, 64, 96, 33, 96)]
    want = [eng.forward(b).clone() for b in batches]
    torch.cuda.synchronize()
    handles = [eng.forward_pipelined(b) for b in batches]
    got = [h.result() for h in reversed(handles)][::-1]
    torch.cuda.synchronize()
    for w, o in zip(want, got):
        assert torch.equal(w, o)
    u8 = (torch.rand(70, 3, 224, 224, generator=g) * 255).to(torch.uint8).cuda()
    assert torch.equal(eng.forward_pipelined(u8).result(), eng.forward(u8))
    with pytest.raises(ValueError):
        eng.forward_pipelined(torch.zeros(2, 3, 32, 32, device="cuda"))


def test_depth_raised_on_a_live_engine():
    """`batches_in_flight` is read on every call: raised from 2 to 3 between calls, the slots are rebuilt (three new
    streams, nothing of the old ones still running) and every batch still comes back as forward() returns it."""
    spec = spec_for("ViT-B-32", "openai")
    eng = VitEngine(spec, random_state_dict(spec, 0), max_batch=8)
    g = torch.Generator().manual_seed(9)
    batches = [torch.randn(8, 3, 224, 224, generator=g).cuda() for _ in range(3)]
    want = [eng.forward(b).clone() for b in batches]
    torch.cuda.synchronize()
    assert len(eng._slots) == 0
    handles = [eng.forward_pipelined(b) for b in batches]
    assert len(eng._slots) == 2
    for w, h in zip(want, handles):
        assert torch.equal(h.result(), w)
    eng.batches_in_flight = 3
    handles = [eng.forward_pipelined(b) for b in batches + batches[:1]]
    assert len(eng._slots) == 3
    for w, h in reversed(list(zip(want + want[:1], handles))):
        assert torch.equal(h.result(), w)
    # a result handle keeps its embeddings and a copy stream, not the engine: weights and workspaces go with the last name
    import weakref
    alive = weakref.ref(eng)
    del eng
    assert alive() is None and handles[0].result().shape == (8, 512)

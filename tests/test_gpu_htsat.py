"""-m gpu: HP-1 audio parity — HTSAT HIP kernels (through the C ABI) against the fp32 CPU oracle and
the committed golden vectors.  Tolerance (BASELINE.json north_star): cosine within 1e-3."""
import numpy as np
import pytest
import torch

from oracle import htsat_ref
from wise_amd.feature.feature_extractor_factory import FeatureExtractorFactory
from wise_amd.feature.htsat import HtsatEngine, checkpoint_like_htsat_state_dict, random_htsat_state_dict

pytestmark = pytest.mark.gpu


def cosine(a, b):
    a = a.double(); b = b.double()
    return ((a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))).min().item()


@pytest.fixture(scope="module")
def engine():
    return HtsatEngine(random_htsat_state_dict(0), max_batch=4, max_samples=480000)


@pytest.fixture(scope="module")
def waves():
    rng = np.random.default_rng(4)  # same stream as oracle/make_golden_htsat.py
    w4 = torch.from_numpy((0.1 * rng.standard_normal((2, 192000))).astype(np.float32))
    w10 = torch.from_numpy((0.1 * rng.standard_normal((1, 480000))).astype(np.float32))
    return w4, w10


def test_frontend_logmel_bn(engine, waves, golden_dir):
    """STFT power -> Slaney mel -> dB -> folded BatchNorm, against the oracle's explicit-DFT front-end."""
    w4, _ = waves
    sd = random_htsat_state_dict(0)
    engine.forward(w4)
    got = engine.tap(0, 2 * 601, 64).cpu().reshape(2, 601, 64)
    mel = htsat_ref.logmel(w4)
    g = np.load(golden_dir / "htsat.npz")
    assert np.allclose(mel[:, :8, :].numpy(), g["mel_head"], atol=1e-4)
    pre = "base.htsat."
    ref = (mel - sd[pre + "bn0.running_mean"]) / torch.sqrt(sd[pre + "bn0.running_var"] + 1e-5) * \
        sd[pre + "bn0.weight"] + sd[pre + "bn0.bias"]
    assert (got - ref).abs().max().item() <= 2e-3  # dB values of O(30), fp32 FFT vs fp32 DFT
    assert cosine(got.reshape(-1, 64), ref.reshape(-1, 64)) >= 1 - 1e-6


def test_golden_4s_clips(engine, waves, golden_dir):
    w4, _ = waves
    g = np.load(golden_dir / "htsat.npz")
    out = engine.forward(w4).cpu()
    assert out.shape == (2, 1024) and out.dtype == torch.float32
    assert torch.allclose(out.norm(dim=1), torch.ones(2), atol=1e-5)
    c = cosine(out, torch.from_numpy(g["out"]))
    assert c >= 1 - 1e-3, c
    # residual stream after stage 4 (before the final norm): first 4 tokens of each clip
    x = engine.tap(1, 2 * 64, 768).cpu().reshape(2, 64, 768)
    assert cosine(x[:, :4, :].reshape(-1, 768), torch.from_numpy(g["tap4"]).reshape(-1, 768)) >= 1 - 1e-3


@pytest.mark.parametrize("fold", [True, False])
def test_checkpoint_like_golden(golden_dir, fold):
    """(both with stages 2 - 4's LayerNorms folded into their GEMMs over a hi + lo residual stream — the default — and without)
    Parity on weights with the statistics of trained checkpoints (massive channels switched on by fc2 biases, log-normal
    LayerNorm gains, near one-hot window attention): the oracle pinned to transformers' ClapAudioModel on the same
    weights, the bf16 HIP path held to the fp32 contract of src/feature/microsoft_clap.py:49-50 at cosine >= 1 - 1e-3."""
    g = np.load(golden_dir / "htsat_stress.npz")
    assert float(g["largest_residual"]) >= 40.0
    eng = HtsatEngine(checkpoint_like_htsat_state_dict(int(g["weight_seed"])), max_batch=2, max_samples=192000, ln_fold=fold)
    assert eng.ln_fold is fold
    rng = np.random.default_rng(int(g["wave_seed"]))
    wave = torch.from_numpy((0.1 * rng.standard_normal((2, 192000))).astype(np.float32))
    out = eng.forward(wave).cpu()
    c = cosine(out, torch.from_numpy(g["out"]))
    assert c >= 1 - 1e-3, c
    x = eng.tap(1, 2 * 64, 768).cpu().reshape(2, 64, 768)
    assert cosine(x[:, :4, :].reshape(-1, 768), torch.from_numpy(g["tap4"]).reshape(-1, 768)) >= 1 - 1e-3


@pytest.mark.parametrize("stress", [False, True])
def test_golden_with_the_one_kernel_mlp(waves, golden_dir, stress):
    """wise_htsat_forward2 flags bit 1: the MLPs of stages 2 and 3 as one kernel each (wise_mlp_stream), on the seeded and on
    the checkpoint-like weights, against the same golden vectors at the same tolerance"""
    if stress:
        g = np.load(golden_dir / "htsat_stress.npz")
        sd = checkpoint_like_htsat_state_dict(int(g["weight_seed"]))
        rng = np.random.default_rng(int(g["wave_seed"]))
        wave = torch.from_numpy((0.1 * rng.standard_normal((2, 192000))).astype(np.float32))
    else:
        g = np.load(golden_dir / "htsat.npz")
        sd, wave = random_htsat_state_dict(0), waves[0]
    eng = HtsatEngine(sd, max_batch=4, max_samples=480000, ln_fold=False, mlp_stream=True, attn_stream=False)
    assert eng.mlp_stream and eng._flags == 2
    out = eng.forward(wave).cpu()
    assert cosine(out, torch.from_numpy(g["out"])) >= 1 - 1e-3
    x = eng.tap(1, 2 * 64, 768).cpu().reshape(2, 64, 768)
    assert cosine(x[:, :4, :].reshape(-1, 768), torch.from_numpy(g["tap4"]).reshape(-1, 768)) >= 1 - 1e-3
    plain = HtsatEngine(sd, max_batch=4, max_samples=480000, ln_fold=False, mlp_stream=False, attn_stream=False).forward(wave).cpu()
    assert cosine(out, plain) >= 1 - 1e-4


@pytest.mark.parametrize("stress", [False, True])
def test_golden_with_the_one_kernel_attention(waves, golden_dir, stress):
    """wise_htsat_forward2 flags bit 2 (with bit 1): norm1 + QKV + window attention of stages 2 and 3 as one kernel each
    (wise_swin_qkv_attn), shifted and unshifted blocks, against the same golden vectors at the same tolerance"""
    if stress:
        g = np.load(golden_dir / "htsat_stress.npz")
        sd = checkpoint_like_htsat_state_dict(int(g["weight_seed"]))
        rng = np.random.default_rng(int(g["wave_seed"]))
        wave = torch.from_numpy((0.1 * rng.standard_normal((2, 192000))).astype(np.float32))
    else:
        g = np.load(golden_dir / "htsat.npz")
        sd, wave = random_htsat_state_dict(0), waves[0]
    eng = HtsatEngine(sd, max_batch=4, max_samples=480000, ln_fold=False, mlp_stream=True, attn_stream=True)
    assert eng.attn_stream and eng._flags == 6
    out = eng.forward(wave).cpu()
    assert cosine(out, torch.from_numpy(g["out"])) >= 1 - 1e-3
    x = eng.tap(1, 2 * 64, 768).cpu().reshape(2, 64, 768)
    assert cosine(x[:, :4, :].reshape(-1, 768), torch.from_numpy(g["tap4"]).reshape(-1, 768)) >= 1 - 1e-3
    plain = HtsatEngine(sd, max_batch=4, max_samples=480000, ln_fold=False, mlp_stream=False, attn_stream=False).forward(wave).cpu()
    assert cosine(out, plain) >= 1 - 1e-4
    only = HtsatEngine(sd, max_batch=4, max_samples=480000, ln_fold=False, mlp_stream=False, attn_stream=True)
    assert only._flags == 4 and cosine(only.forward(wave).cpu(), plain) >= 1 - 1e-4


def test_golden_4s_clips_without_the_fold(waves, golden_dir):
    """the unfolded form (LayerNorm launches, fp32 rows) stays available and inside the same tolerance"""
    w4, _ = waves
    g = np.load(golden_dir / "htsat.npz")
    eng = HtsatEngine(random_htsat_state_dict(0), max_batch=4, max_samples=480000, ln_fold=False)
    out = eng.forward(w4).cpu()
    assert cosine(out, torch.from_numpy(g["out"])) >= 1 - 1e-3
    x = eng.tap(1, 2 * 64, 768).cpu().reshape(2, 64, 768)
    assert cosine(x[:, :4, :].reshape(-1, 768), torch.from_numpy(g["tap4"]).reshape(-1, 768)) >= 1 - 1e-3
    folded = HtsatEngine(random_htsat_state_dict(0), max_batch=4, max_samples=480000, ln_fold=True).forward(w4).cpu()
    assert cosine(out, folded) >= 1 - 1e-4


def test_golden_10s_clip_and_batch_independence(engine, waves, golden_dir):
    w4, w10 = waves
    g = np.load(golden_dir / "htsat.npz")
    out10 = engine.forward(w10).cpu()
    assert cosine(out10, torch.from_numpy(g["out10"])) >= 1 - 1e-3
    # a clip's embedding does not depend on its batch (deterministic kernels, no cross-clip mixing)
    a = engine.forward(w4).cpu()
    b = engine.forward(w4[1:2]).cpu()
    assert torch.equal(a[1:2], b)
    # odd batch (row padding path)
    c = engine.forward(torch.cat([w4, w4[:1]], dim=0)).cpu()
    assert torch.equal(c[:2], a) and torch.equal(c[2], a[0])


def test_batch128_of_10s_clips(waves, golden_dir):
    """BASELINE cfg-5 at its own size: 128 clips x 480000 samples (10 s @48 kHz; the reference feeds
    microsoft_clap.py:45-51 one 4-s segment at a time).  Clip 0 is the golden 10-s clip and must match the oracle's
    vector; every row unit-norm; a clip's embedding is the one it gets alone (batch independence, bit for bit); the
    pipelined form returns the same bits."""
    _, w10 = waves
    g = np.load(golden_dir / "htsat.npz")
    B, N = 128, 480000
    eng = HtsatEngine(random_htsat_state_dict(0), max_batch=B, max_samples=N)
    w = 0.1 * torch.randn(B, N, device="cuda", generator=torch.Generator("cuda").manual_seed(4))
    w[0] = w10[0].cuda()
    out = eng.forward(w)
    assert out.shape == (B, 1024) and out.dtype == torch.float32
    assert torch.allclose(out.norm(dim=1).cpu(), torch.ones(B), atol=1e-5)
    assert cosine(out[:1].cpu(), torch.from_numpy(g["out10"])) >= 1 - 1e-3
    for b in (0, 1, 77, 127):
        assert torch.equal(eng.forward(w[b:b + 1]), out[b:b + 1])
    assert torch.equal(eng.forward(w[40:103]), out[40:103])           # a ragged sub-batch
    assert torch.equal(eng.forward_pipelined(w).result(), out)
    # the oracle itself on one more clip of the batch (a few seconds of CPU)
    ref = htsat_ref.htsat_forward(random_htsat_state_dict(0), w[127:128].cpu())
    assert cosine(out[127:128].cpu(), ref) >= 1 - 1e-3


def test_microsoft_clap_plugin_surface(waves, golden_dir):
    """Through the reference's plugin API (microsoft_clap.py:33-51): preprocess_audio -> extract_audio_features."""
    w4, _ = waves
    fx = FeatureExtractorFactory("microsoft/clap/2023/seeded-0")
    stereo = torch.stack([w4[0], w4[0]], dim=0)  # [2, N] -> mono mix == w4[0]
    pre = fx.preprocess_audio(stereo)
    assert pre.shape == (1, 1, 192000)
    feats = fx.extract_audio_features(pre)
    assert isinstance(feats, np.ndarray) and feats.shape == (1, 1024) and feats.dtype == np.float32
    g = np.load(golden_dir / "htsat.npz")
    assert cosine(torch.from_numpy(feats), torch.from_numpy(g["out"][:1])) >= 1 - 1e-3
    # the reference's own test feeds 408700 samples and checks the dim only (test_feature_extractor.py:37-41)
    long = fx.extract_audio_features(fx.preprocess_audio(torch.rand(1, 408700)))
    assert long.shape == (1, 1024)


def test_two_batches_in_flight_equal_serial():
    """HtsatEngine.forward_pipelined: two forwards overlapping on two streams return what one forward returns alone,
    bit for bit, every time (the STFT kernel once did not: see the note at the top of csrc/htsat_frontend.hip)."""
    B, N = 16, 480000
    eng = HtsatEngine(random_htsat_state_dict(0), max_batch=B, max_samples=N)
    w = 0.1 * torch.randn(B, N, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    ref = eng.forward(w).clone()
    for _ in range(6):
        pending = [eng.forward_pipelined(w) for _ in range(4)]
        for p in pending:
            assert torch.equal(p.result(), ref)


def test_frontend_beside_matrix_kernels():
    """The log-mel front end run while another stream keeps the matrix cores busy (the fused HTSAT MLP, and a bare
    MFMA loop sized to share compute units with it) is bit-identical to the front end run alone."""
    import ctypes

    from wise_amd import _lib
    lib = _lib.lib()
    dbg = _lib.load_debug()   # only the bare-MFMA neighbour comes from the debug twin; everything under test is the product's
    dbg.wise_debug_neighbour.restype = ctypes.c_int
    dbg.wise_debug_neighbour.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3
    B, N, Fc = 16, 480000, 1024
    eng = HtsatEngine(random_htsat_state_dict(0), max_batch=B, max_samples=N)
    w = 0.1 * torch.randn(B, N, device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    need = lib.wise_htsat_workspace_bytes(B, N)
    wss = [torch.empty(need, dtype=torch.uint8, device="cuda") for _ in range(8)]
    out = torch.empty(B, 1024, device="cuda")
    s_front, s_other = torch.cuda.Stream(), torch.cuda.Stream()
    M = 131072
    x = torch.randn(M, 96, device="cuda")
    lnw, lnb = torch.ones(96, device="cuda"), torch.zeros(96, device="cuda")
    W1 = (0.05 * torch.randn(384, 96, device="cuda")).bfloat16(); b1 = torch.zeros(384, device="cuda")
    W2 = (0.05 * torch.randn(96, 384, device="cuda")).bfloat16(); b2 = torch.zeros(96, device="cuda")
    src = torch.zeros(1024, dtype=torch.int32, device="cuda"); sink = torch.zeros(4, dtype=torch.int32, device="cuda")
    P = lambda t: t.data_ptr()
    neighbours = {
        "fused MLP": lambda: lib.wise_mlp96_fused(P(x), P(lnw), P(lnb), P(W1), P(b1), P(W2), P(b2), M, 1e-5,
                                                  s_other.cuda_stream),
        "MFMA loop": lambda: dbg.wise_debug_neighbour(3, 2048, 61440, 64, P(src), P(sink), s_other.cuda_stream),
    }

    def front(ws):
        _lib.check(lib.wise_htsat_forward(eng.wb.data_ptr(), eng.pf.data_ptr(), w.data_ptr(), B, N, out.data_ptr(),
                                          ws.data_ptr(), ws.numel(), s_front.cuda_stream), "front end")

    def mel_of(ws):
        mel = torch.empty(B * Fc, 64, device="cuda")
        _lib.check(lib.wise_htsat_tap(0, ws.data_ptr(), B, N, mel.data_ptr(), mel.numel(), _lib.stream_ptr()), "tap")
        torch.cuda.synchronize()
        return mel

    # (whole forwards: the log-mel image stays in the workspace after the Swin stages and is tapped from there)
    torch.cuda.synchronize()
    front(wss[0]); torch.cuda.synchronize()
    alone = mel_of(wss[0])
    for name, fn in neighbours.items():
        for ws in wss:
            ws[:B * Fc * 256].zero_()
        torch.cuda.synchronize()
        for ws in wss:
            for _ in range(3):
                _lib.check(fn(), name)
            front(ws)
        torch.cuda.synchronize()
        wrong = sum(0 if torch.equal(mel_of(ws), alone) else 1 for ws in wss)
        assert wrong == 0, f"{wrong} of {len(wss)} front ends differ beside {name}"


@pytest.mark.parametrize("order", ["SLSLSL", "SSLLSS"])
def test_slot_workspace_regrows_between_batches(waves, order):
    """4-s and 10-s batches (S, L) through forward_pipelined, six submitted and none collected in between; every result
    is forward()'s, bit for bit.  The two slots take the submissions in turn.  SLSLSL: slot 0 gets every short batch and
    slot 1 every long one, each sized once.  SSLLSS: each slot gets short, long, short, so its workspace is too small
    for its second batch and is replaced while its first and the other slot's batch may still run, and is kept, larger than
    needed, for its third."""
    w4, w10 = waves
    short, long = w4.cuda(), torch.cat([w10, w10.flip(1)]).cuda()
    eng = HtsatEngine(random_htsat_state_dict(0), max_batch=2, max_samples=short.shape[1])
    want = {"S": eng.forward(short).clone(), "L": eng.forward(long).clone()}
    torch.cuda.synchronize()
    handles = [eng.forward_pipelined(short if c == "S" else long) for c in order]
    sizes = [sl["ws"].numel() for sl in eng._slots]
    assert (sizes[0] == sizes[1]) == (order == "SSLLSS")        # both slots grew to the long batch's size, or neither did
    for c, h in zip(order, handles):
        assert torch.equal(h.result(), want[c])

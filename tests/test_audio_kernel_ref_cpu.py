"""No GPU: tests/audio_kernel_ref.py held to account.

  ledger      the table has a case for every instantiation and form the audio towers launch, and block 1's cases visit every
              (ring phase t2 mod 3, warm | cold) pair of conv_block1_kernel's run walk
  oracle      in float32, on the table's own inputs, each restatement agrees with the matching piece of oracle/htsat_ref.py or
              oracle/cnn14_ref.py (the references pinned to the upstream models).  Where the oracle has no function for the piece
              alone, the piece is cut out of the larger one with neutral weights: an MLP whose fc2 is zero leaves swin_block's
              attention half, an identity reduction leaves patch_merge's gather + LayerNorm, linear1 = I and linear2 = 0 leave
              projection's LayerNorm.  cnn14_ref has block 1 and the pooling head only as lines of cnn14_embedding: the same torch
              calls (conv2d, its _bn, relu, avg_pool2d) are made here with an identity BatchNorm.
  checker     the exact output passes every case; every planted fault fails on a case of its kernel
  the 1 % cap bf16(ref32) differs from bf16(want64) in under 0.1 % of the elements of every bf16 case: a correct fp32 kernel is
              a factor of ten away from the cap on flipped roundings"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cnn14_ref, htsat_ref
from tests import audio_kernel_ref as ak
from tests import swin_window_ref as sw

ALL = [(k, i) for k, cs in ak.CASES.items() for i in range(len(cs))]
F64 = torch.float64


@functools.lru_cache(maxsize=None)
def problem(kernel, i):
    return ak.build(kernel, ak.CASES[kernel][i])


def find(kernel, **kw):
    """the problem of the first case of `kernel` with these parameters"""
    for i, c in enumerate(ak.CASES[kernel]):
        if all(c[k] == v for k, v in kw.items()):
            return problem(kernel, i)
    raise KeyError((kernel, kw))


def fails(p, out):
    """the checker refuses `out` (float64 [rows, cols], or a whole buffer)"""
    full = out if out.shape[0] == p.rows + ak.GUARD else ak.as_output(out, p.out_dtype)
    assert tuple(full.shape) == (p.rows + ak.GUARD, p.cols) and full.dtype == p.out_dtype      # refused for its values, not its form
    with pytest.raises(AssertionError, match=p.what):
        ak.check(p, full)
    return True


# ------------------------------------------------------------------------------------------------ ledger
def test_the_table_covers_what_the_towers_launch():
    seen = {ak.instantiation(k, c) for k, cs in ak.CASES.items() for c in cs}
    assert seen >= {"embed_tok_kernel", "swin96_block_attn_kernel<0>", "swin96_block_attn_kernel<4>", "merge_ln_kernel<2> fp32",
                    "merge_ln_kernel<3> fp32", "merge_ln_kernel<3> hi+lo", "merge_ln_kernel<6> fp32", "merge_ln_kernel<6> hi+lo",
                    "latent_kernel fp32", "latent_kernel hi+lo", "proj_ln_norm_kernel", "conv_block1_kernel<0>",
                    "head_pool_kernel"}
    # the issue's table, by count: nothing dropped
    assert {k: len(cs) for k, cs in ak.CASES.items()} == {"embed": 12, "swin96": 7, "merge_ln": 12, "latent": 4,
                                                          "proj_ln_norm": 3, "block1": 5, "head_pool": 4}
    for c in ak.CASES["merge_ln"]:
        if c["hilo"]:
            assert problem("merge_ln", ak.CASES["merge_ln"].index(c)).lo_off == ak.ceil128(c["B"] * c["H"] ** 2) * c["C"]


def test_block1_cases_visit_every_ring_phase_warm_and_cold():
    walks = {(c["B"], c["T"], c["chunk"]): ak.block1_walk(c["B"], c["T"], c["chunk"]) for c in ak.CASES["block1"]}
    assert set().union(*walks.values()) == {(ph, s) for ph in range(3) for s in ("cold", "warm")}
    assert all(s == "cold" for _, s in walks[(2, 67, 0)])                       # runs of one row: every tile cold
    assert walks[(2, 67, 188)] == {(ph, "warm") for ph in range(3)} | {(0, "cold")}   # one run; cold at each clip's first tile
    assert ak.block1_chunk(3, 347, 0) == 2 and ak.block1_chunk(1, 32, 0) == 1
    assert ak.block1_chunk(128, 1501, 0) == 188                                 # the benchmark's shape


def test_the_sampling_position_is_the_same_in_both_divisions():
    """float32((Fc - 1) / 1023) is what the kernel's fp32 division gives, for every Fc of the table"""
    for fc in ak.EMBED_FC:
        assert np.float32(fc - 1) / np.float32(1023) == np.float32((fc - 1) / 1023)


# ------------------------------------------------------------------------------------------------ the restatements are the oracle's
def close(a, b, rtol=1e-4, atol=1e-4):
    a, b = a.to(F64), b.to(F64)
    assert a.shape == b.shape
    assert torch.allclose(a, b, rtol=rtol, atol=atol), float((a - b).abs().max())


@pytest.mark.parametrize("fc", ak.EMBED_FC)
def test_embed_is_the_oracles(fc):
    p = find("embed", Fc=fc)
    r = p.raw
    pre = "base.htsat."
    sd = {pre + "bn0.running_mean": torch.zeros(64), pre + "bn0.running_var": torch.full((64,), 1 - 1e-5),
          pre + "bn0.weight": torch.ones(64), pre + "bn0.bias": torch.zeros(64),
          pre + "patch_embed.proj.weight": r["pw"].reshape(96, 1, 4, 4), pre + "patch_embed.proj.bias": r["pb"],
          pre + "patch_embed.norm.weight": r["lnw"], pre + "patch_embed.norm.bias": r["lnb"],
          pre + "norm.weight": torch.ones(96), pre + "norm.bias": torch.zeros(96)}
    taps = []
    htsat_ref.body_forward(sd, r["mel"], taps=taps, stages=0)
    close(p.ref32, taps[0].reshape(-1, 96), atol=2e-4)
    img = htsat_ref.mel_to_image(r["mel"])
    close(ak.embed_fold(ak.embed_resample(r["mel"], torch.float32)), img, atol=1e-5)


@pytest.mark.parametrize("shift", [0, 4])
def test_swin96_is_the_oracles_attention_half(shift):
    p = find("swin96", shift=shift, B=2)
    r, pre = p.raw, "b."
    sd = {pre + "norm1.weight": r["n1w"], pre + "norm1.bias": r["n1b"], pre + "attn.qkv.weight": r["wqkv"].float(),
          pre + "attn.qkv.bias": r["qkvb"], pre + "attn.relative_position_bias_table": p.table,
          pre + "attn.proj.weight": r["wproj"].float(), pre + "attn.proj.bias": r["pb"],
          pre + "norm2.weight": torch.ones(96), pre + "norm2.bias": torch.zeros(96),
          pre + "mlp.fc1.weight": torch.zeros(384, 96), pre + "mlp.fc1.bias": torch.zeros(384),
          pre + "mlp.fc2.weight": torch.zeros(96, 384), pre + "mlp.fc2.bias": torch.zeros(96)}
    ref = htsat_ref.swin_block(r["x"].reshape(2, 4096, 96), pre, sd, 64, 64, 4, shift).reshape(-1, 96)
    close(p.exact, ref, rtol=1e-4, atol=1e-3)       # (the outlier element is 1e4: one fp32 step there is 1e-3)


@pytest.mark.parametrize("i", [i for i, c in enumerate(ak.CASES["merge_ln"]) if not c["hilo"]])
def test_merge_ln_is_the_oracles(i):
    p, c = problem("merge_ln", i), ak.CASES["merge_ln"][i]
    sd = {"d.norm.weight": p.raw["w"], "d.norm.bias": p.raw["b"], "d.reduction.weight": torch.eye(4 * c["C"])}
    ref = htsat_ref.patch_merge(p.raw["x"].reshape(c["B"], -1, c["C"]), "d.", sd, c["H"], c["H"])
    close(p.ref32, ref.reshape(-1, 4 * c["C"]), atol=2e-3)     # (the outlier row: values of 40 after the LayerNorm)


def test_latent_and_projection_are_the_oracles():
    p = find("latent", hilo=0, B=3)
    close(p.ref32, htsat_ref.layer_norm(p.raw["x"].reshape(3, 64, 768), p.raw["nw"], p.raw["nb"]).mean(dim=1))
    p = find("proj_ln_norm", B=5)
    sd = {"projection.linear1.weight": torch.eye(1024), "projection.linear2.weight": torch.zeros(1024, 1024),
          "projection.layer_norm.weight": p.raw["lw"], "projection.layer_norm.bias": p.raw["lb"]}
    out = htsat_ref.projection(sd, p.raw["e"])
    close(p.ref32, out / torch.norm(out, dim=-1, keepdim=True), atol=1e-6)
    close(p.ref32, torch.from_numpy(_cnn14_projection(sd, p.raw["e"])), atol=1e-6)


def _cnn14_projection(sd, e):
    out = cnn14_ref.projection(sd, e)
    return (out / out.norm(dim=-1, keepdim=True)).numpy()


def test_block1_and_head_pool_are_the_oracles():
    p = find("block1", B=2, T=67, chunk=0)
    r = p.raw
    one = {"running_mean": torch.zeros(64), "running_var": torch.full((64,), 1 - 1e-5), "weight": torch.ones(64)}
    sd = {"bn1." + k: v for k, v in one.items()} | {"bn2." + k: v for k, v in one.items()} | {"bn1.bias": r["s0"], "bn2.bias": r["bias2"]}
    w2 = r["Wt"].float().reshape(64, 3, 3, 64).permute(0, 3, 1, 2)
    x = r["mel"][:, None]                                                   # the lines of cnn14_ref.cnn14_embedding, block 1
    x = F.relu(cnn14_ref._bn(F.conv2d(x, r["w0"].reshape(64, 1, 3, 3), padding=1), sd, "bn1."))
    x = F.relu(cnn14_ref._bn(F.conv2d(x, w2, padding=1), sd, "bn2."))
    x = F.avg_pool2d(x, kernel_size=2)
    got = ak.block1_ref(r["mel"], r["w0"], r["s0"], r["Wt"], r["bias2"], torch.float32, mid_bf16=False)
    close(got, x.permute(0, 2, 3, 1).reshape(-1, 64), atol=1e-4)
    # and the rounding of the tensor between the convolutions moves the result by bf16 noise, no more
    assert float((p.want - got.double()).abs().max()) < 2e-2
    p = find("head_pool", T=7)
    y = p.raw["x"].float().permute(0, 3, 1, 2)                              # [B, C, T, F] as the oracle holds it
    y = y.mean(dim=3)
    close(p.ref32, y.max(dim=2).values + y.mean(dim=2), atol=1e-5)


# ------------------------------------------------------------------------------------------------ the checker
@pytest.mark.parametrize("kernel,i", ALL, ids=[ak.case_id(k, ak.CASES[k][i]) for k, i in ALL])
def test_exact_outputs_pass_and_the_cap_is_far(kernel, i):
    p = problem(kernel, i)
    ak.check(p, ak.as_output(p.want, p.out_dtype))
    if p.kind == "swin":
        ak.check(p, ak.as_output(p.exact, p.out_dtype))            # n away from `rounded`: inside 2 n
    if p.kind == "bf16":
        flips = ak.flip_share(p.ref32.to(torch.bfloat16), p.want)
        assert flips < 0.001, f"{p.what}: bf16(ref32) != bf16(want64) in {100 * flips:.3f} % of the elements"
    # every kernel: one NaN, one overwritten guard row
    full = ak.as_output(p.want, p.out_dtype)
    full[p.rows // 2, p.cols // 2] = float("nan")
    assert fails(p, full)
    full = ak.as_output(p.want, p.out_dtype)
    full[p.rows + 1, 3] = 0.5
    assert fails(p, full)
    # ... and one wrong row out of all of them
    full = ak.as_output(p.want, p.out_dtype)
    full[p.rows - 1] = full[p.rows - 1] * 1.05 + 0.05
    assert fails(p, full)


def _resample(mel, index):
    """bicubic resampling with tap j of clip b read at row index(b, j, i0 - 1 + j) of the flat [B*Fc, 64] log-mel"""
    B, Fc, _ = mel.shape
    i0, t = ak.bicubic_positions(Fc)
    w, flat = ak.cubic_weights(t, F64), mel.double().reshape(B * Fc, 64)
    out = torch.zeros(B, 1024, 64, dtype=F64)
    for b in range(B):
        for j in range(4):
            out[b] += flat[index(b, j, i0 - 1 + j)] * w[:, j].view(1024, 1)
    return out


@pytest.mark.parametrize("fault", ["tap off by one", "no clamp at the last frame", "r and f swapped in the fold"])
def test_embed_faults(fault):
    for fc in (5, 601):
        p = find("embed", Fc=fc, form=0)
        r, B = p.raw, 2
        clamp = lambda b, j, a: b * fc + torch.clamp(a, 0, fc - 1)
        if fault == "tap off by one":
            m = _resample(r["mel"], lambda b, j, a: clamp(b, j, a + (j == 3)))
        elif fault == "no clamp at the last frame":         # the read goes into the next clip
            m = _resample(r["mel"], lambda b, j, a: torch.clamp(b * fc + torch.clamp(a, min=0), max=B * fc - 1))
        else:
            m = _resample(r["mel"], clamp)
        assert (fault != "r and f swapped in the fold") == (not torch.equal(m, ak.embed_resample(r["mel"], F64)))
        img = ak.embed_fold(m) if fault != "r and f swapped in the fold" else m.reshape(B, 4, 256, 64).permute(0, 3, 1, 2).reshape(B, 256, 256)
        assert fails(p, ak.embed_patch_ln(img, r["pw"], r["pb"], r["lnw"], r["lnb"]))


def _swin_from(p, o):
    return torch.from_numpy(ak.swin_proj(p.raw["x"], o, p.raw["wproj"], p.raw["pb"]))


def _roll(a, B, C, s):
    return np.roll(a.reshape(B, 64, 64, C), (s, s), (1, 2)).reshape(-1, C)


def test_swin96_faults():
    p = find("swin96", shift=4, B=1, grid=0)
    r = p.raw
    relb = r["relb"].double().numpy()
    qkv = ak.swin_qkv(r["x"], r["n1w"], r["n1b"], r["wqkv"], r["qkvb"], False)
    assert torch.allclose(_swin_from(p, ak.swin_attention(qkv, relb, 1, 4, False)), p.exact)
    # bias transposed: query and key swapped
    assert fails(p, _swin_from(p, ak.swin_attention(qkv, relb.transpose(0, 2, 1), 1, 4, False)))
    # mask dropped: the shifted attention is the unshifted one on rolled rows, rolled back — without the region mask
    assert fails(p, _swin_from(p, _roll(sw.window_attention(_roll(qkv, 1, 288, -4), relb, 1, 64, 96, 0), 1, 96, 4)))
    # shift applied with the other sign (mask kept): roll by +4 where -4 belongs, and back by -4
    assert fails(p, _swin_from(p, _roll(sw.window_attention(_roll(qkv, 1, 288, 8), relb, 1, 64, 96, 4), 1, 96, -8)))
    # two heads swapped
    assert fails(p, _swin_from(p, ak.swin_attention(qkv, relb[[1, 0, 2, 3]], 1, 4, False)))
    for shift in (0, 4):
        p = find("swin96", shift=shift, B=1, grid=24)
        win = sw.partition(np.arange(4096).reshape(1, 64, 64, 1), 64, shift)[0, :, :, 0]      # [window, token] -> row
        # two rows of one window swapped
        out = p.exact.clone()
        a, b = int(win[37, 5]), int(win[37, 6])
        out[[a, b]] = out[[b, a]]
        assert fails(p, out)
        # the second trip of workgroup 0 (window 24) reusing the first trip's rows (window 0)
        out, delta = p.exact.clone(), p.exact - p.raw["x"].double()
        out[win[24]] = p.raw["x"].double()[win[24]] + delta[win[0]]
        assert fails(p, out)


def test_merge_ln_and_latent_faults():
    for i, c in enumerate(ak.CASES["merge_ln"]):
        p = problem("merge_ln", i)
        B, H, C = c["B"], c["H"], c["C"]
        x = (p.raw["x_val"] if c["hilo"] else p.raw["x"].double()).reshape(B, H, H, C)
        if H > 2:       # segments 1 and 2 swapped: the transposed image, transposed back
            out = ak.merge_ln_ref(x.transpose(1, 2), p.raw["w"], p.raw["b"]).reshape(B, H // 2, H // 2, 4 * C).transpose(1, 2)
            assert fails(p, out.reshape(-1, 4 * C))
        if c["hilo"]:   # lo dropped: every case sees it
            assert fails(p, ak.merge_ln_ref(p.raw["hi"].double(), p.raw["w"], p.raw["b"]))
    for i, c in enumerate(ak.CASES["latent"]):
        p = problem("latent", i)
        x = (p.raw["x_val"] if c["hilo"] else p.raw["x"].double()).reshape(c["B"], 64, 768)
        assert fails(p, ak.layer_norm(x, p.raw["nw"], p.raw["nb"])[:, :63].mean(dim=1))          # mean over 63 tokens
        assert fails(p, ak.layer_norm(x.mean(dim=1), p.raw["nw"], p.raw["nb"]))                  # LayerNorm after the mean
        if c["hilo"]:
            assert fails(p, ak.latent_ref(p.raw["hi"].double(), p.raw["nw"], p.raw["nb"]))


def test_proj_ln_norm_faults():
    p = find("proj_ln_norm", B=4)
    e = p.raw["e"].double()
    y = ak.layer_norm(e, p.raw["lw"], p.raw["lb"], eps=1e-6)
    assert fails(p, y / y.norm(dim=-1, keepdim=True))                                            # eps 1e-6
    assert fails(p, ak.layer_norm(e, p.raw["lw"], p.raw["lb"]))                                  # no normalise


def test_block1_faults():
    def mid_of(p):
        r = p.raw
        return ak.block1_conv1(r["mel"], r["w0"], r["s0"], F64)

    def out_of(p, padded):
        return ak.block1_pool(ak.block1_conv2(padded, p.raw["Wt"], p.raw["bias2"]))

    pad = lambda m: F.pad(m, (1, 1, 1, 1))
    # bottom padding row taken as the clamped last row instead of zeros: an even T reads it
    p = find("block1", T=66)
    mid = mid_of(p)
    assert torch.equal(out_of(p, pad(mid)), p.want)
    padded = pad(mid)
    padded[:, :, -1, 1:-1] = mid[:, :, -1, :]
    assert fails(p, out_of(p, padded))
    # a stale ring slot: one warm tile (clip 0, pooled row 5) sees row t - 2 where row t = 12, its newest, belongs
    p = find("block1", T=67, chunk=188)
    padded = pad(mid_of(p))
    padded[0, :, 13] = padded[0, :, 11]
    out = p.want.clone()
    out[5 * 32:6 * 32] = out_of(p, padded)[5 * 32:6 * 32]
    assert fails(p, out)
    # the first row of clip 1 built from clip 0's last log-mel row where the zero padding belongs
    r = p.raw
    joined = ak.block1_conv1(torch.cat([r["mel"][0, -1:], r["mel"][1]])[None], r["w0"], r["s0"], F64)
    mid = mid_of(p)
    mid[1, :, 0] = joined[0, :, 1]
    assert fails(p, out_of(p, pad(mid)))
    # pooling windows one column off
    y = ak.block1_conv2(pad(mid_of(p)), r["Wt"], r["bias2"])
    assert fails(p, ak.block1_pool(F.pad(y[..., 1:], (0, 1))))


def test_head_pool_fault():
    p = find("head_pool", T=3)
    x = p.raw["x"].double()
    assert fails(p, x.max(dim=1).values.mean(dim=1) + x.mean(dim=(1, 2)))                        # max taken before the mean over F

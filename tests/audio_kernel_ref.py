"""The audio towers' own kernels (csrc/htsat.hip, csrc/cnn14.hip), one by one: the case table, a float64 restatement of each
operation, seeded inputs, and the elementwise checker.  Plain torch / numpy on the CPU: tests/test_gpu_audio_kernels.py runs the
kernels against it through the wise_debug_* twins, tests/test_audio_kernel_ref_cpu.py holds the table, the restatements (against
oracle/htsat_ref.py and oracle/cnn14_ref.py) and the checker (against planted faults) to account without a GPU.

Restatements state the operation, not the kernel's code; each takes the dtype it computes in, so the same text gives want64
(float64) and ref32 (torch float32 on the CPU: the yardstick of what fp32 arithmetic costs):

  embed         bicubic resample in time to 1024 frames (A = -0.75, taps clamped to the clip; the sampling position
                src = float32(t) * float32((Fc - 1) / 1023), its floor and its fraction are fp32 by definition, as in torch's
                upsample_bicubic2d and oracle/htsat_ref.bicubic_time; Fc = 1024 resamples nothing), the fold
                image[r*64 + f][t'] = mel[r*256 + t'][f], the 4x4 / 4 convolution, LayerNorm.  The LayerNorm input is made inside
                the kernel, so this is the one LayerNorm here without a constant and an outlier row of its own.
  swin96        x + proj(window_attention(LN1(x) Wqkv^T + b)) + b_proj in two variants: `exact` rounds nowhere; `rounded` rounds
                to bf16 where swin96_block_attn_kernel stores bf16: the LayerNorm output, q / k / v, the softmax weights and the
                attention output.  Read from the kernel: the weights it rounds are the UNNORMALISED exp(s - max) (in (0, 1]), their
                sum is taken over the unrounded values and divides the product afterwards; `rounded` does the same.
  merge_ln      segments (2i,2j) (2i+1,2j) (2i,2j+1) (2i+1,2j+1), LayerNorm over 4C; the hi + lo form's input IS hi + lo
  latent        LayerNorm per token, mean of the 64 tokens
  proj_ln_norm  LayerNorm, division by the L2 norm
  block1        conv 1 (3x3, zero padding, fp32 weights) + s0, ReLU, rounded to bf16; conv 2 (bf16 weights) + bias2, ReLU; 2x2
                mean, which drops the last frame of an odd T
  head_pool     mean over F, then max over T + mean over T

Guards: every output has GUARD rows behind it prefilled with the NaN pattern of tests/test_gpu_row_kernel_hashes.py, which must
come back untouched; every input is followed by NaN guard rows, so a read past its end shows as a non-finite output."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import htsat_ref
from tests import swin_window_ref as sw

GUARD = 4
BF16_GUARD = 0x7FC1
F32_GUARD = 0x7FC00001
A_CUBIC = -0.75

# ------------------------------------------------------------------------------------------------ the case table
EMBED_FC = (2, 3, 5, 601, 1023, 1024)       # 2, 3, 5: all four taps clamp; 601: a 4 s clip; 1024: no resampling
CASES = {
    "embed": [dict(form=form, B=2, Fc=fc) for form in (0, 1) for fc in EMBED_FC],
    # grid 0 = the tower's rule min(64 B, 512); (1, 24): trips of 3 and 2 (ragged); (9, 0): 576 windows on 512 workgroups
    "swin96": [dict(shift=s, B=b, grid=g) for s in (0, 4) for b, g in ((1, 0), (1, 24), (2, 0)) + (((9, 0),) if s else ())],
    "merge_ln": [dict(hilo=h, B=b, H=hh, C=c) for h in (0, 1)
                 for b, hh, c in ((3, 6, 96), (1, 64, 96), (3, 2, 192), (1, 32, 192), (5, 2, 384), (1, 16, 384))],
    "latent": [dict(hilo=h, B=b) for h in (0, 1) for b in (1, 3)],
    "proj_ln_norm": [dict(B=b) for b in (1, 4, 5)],
    "block1": [dict(B=b, T=t, chunk=c) for b, t, c in ((1, 32, 0), (2, 67, 0), (2, 67, 188), (3, 66, 7), (3, 347, 0))],
    "head_pool": [dict(B=b, T=t, F=f, C=c) for b, t, f, c in ((3, 1, 2, 2048), (2, 3, 2, 2048), (1, 18, 2, 2048), (5, 7, 3, 64))],
}
KIND = {"embed": "f32", "proj_ln_norm": "f32", "merge_ln": "bf16", "latent": "bf16", "head_pool": "bf16", "swin96": "swin",
        "block1": "block1"}


def case_id(kernel, c):
    return kernel + "-" + "-".join(f"{k}{v}" for k, v in c.items())


def ceil128(n):
    return (n + 127) // 128 * 128


def instantiation(kernel, c):
    """what the case launches, named as in the sources (the ledger of tests/test_audio_kernel_ref_cpu.py)"""
    if kernel == "embed":
        return "embed_tok_kernel" if c["form"] == 0 else "embed_kernel"
    if kernel == "swin96":
        return f"swin96_block_attn_kernel<{c['shift']}>"
    if kernel == "merge_ln":
        return f"merge_ln_kernel<{(c['C'] + 63) // 64}> " + ("hi+lo" if c["hilo"] else "fp32")
    if kernel == "latent":
        return "latent_kernel " + ("hi+lo" if c["hilo"] else "fp32")
    return {"proj_ln_norm": "proj_ln_norm_kernel", "block1": "conv_block1_kernel<0>", "head_pool": "head_pool_kernel"}[kernel]


def block1_chunk(B, T, chunk):
    """pooled rows per workgroup: `chunk`, or (0) cnn14::forward's rule"""
    rows2 = B * (T // 2)
    return chunk if chunk else -(-rows2 // min(rows2, 512))


def block1_walk(B, T, chunk):
    """the (t2 mod 3, 'cold' | 'warm') pairs conv_block1_kernel's run walk visits: a workgroup owns `chunk` consecutive pooled
    rows; its first tile and every clip's first tile build all four image rows (cold), the others reuse two (warm)"""
    T2, seen = T // 2, set()
    rows2, chunk = B * T2, block1_chunk(B, T, chunk)
    for r0 in range(0, rows2, chunk):
        r1, cold = min(rows2, r0 + chunk), True
        for g2 in range(r0, r1):
            t2 = g2 % T2
            seen.add((t2 % 3, "cold" if cold else "warm"))
            cold = not (t2 + 1 < T2 and g2 + 1 < r1)
    return seen


# ------------------------------------------------------------------------------------------------ restatements
def layer_norm(x, w, b, eps=1e-5):
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * w.to(x.dtype) + b.to(x.dtype)


def bicubic_positions(Fc):
    """(first tap's neighbour i0 [1024] int64, fraction [1024] float32) of the 1024 output frames: fp32 by definition"""
    src = torch.arange(1024, dtype=torch.float32) * torch.tensor(np.float32((Fc - 1) / 1023))
    fl = torch.floor(src)
    return fl.to(torch.int64), src - fl


def cubic_weights(t, dt):
    """[1024, 4] weights of taps i0 - 1 .. i0 + 2"""
    t, A = t.to(dt), A_CUBIC
    c1 = lambda v: ((A + 2) * v - (A + 3)) * v * v + 1
    c2 = lambda v: ((A * v - 5 * A) * v + 8 * A) * v - 4 * A
    return torch.stack([c2(t + 1), c1(t), c1(1 - t), c2(2 - t)], dim=1)


def embed_resample(mel, dt):
    """[B, Fc, 64] -> [B, 1024, 64]"""
    B, Fc, _ = mel.shape
    m = mel.to(dt)
    if Fc == 1024:
        return m
    i0, t = bicubic_positions(Fc)
    w = cubic_weights(t, dt)
    out = torch.zeros(B, 1024, 64, dtype=dt)
    for j in range(4):
        out += m[:, torch.clamp(i0 - 1 + j, 0, Fc - 1), :] * w[:, j].view(1, 1024, 1)
    return out


def embed_fold(m):
    """[B, 1024, 64] -> the 256 x 256 image: image[r*64 + f][t'] = m[r*256 + t'][f]"""
    B = m.shape[0]
    return m.reshape(B, 4, 256, 64).permute(0, 1, 3, 2).reshape(B, 256, 256)


def embed_patch_ln(img, pw, pb, lnw, lnb):
    """4x4 / 4 convolution (pw [96, 16], pixel p = 4 * row + column of the patch) + LayerNorm -> [B*4096, 96]"""
    B, dt = img.shape[0], img.dtype
    patches = img.reshape(B, 64, 4, 64, 4).permute(0, 1, 3, 2, 4).reshape(B * 4096, 16)
    return layer_norm(patches @ pw.to(dt).t() + pb.to(dt), lnw, lnb)


def embed_ref(mel, pw, pb, lnw, lnb, dt):
    return embed_patch_ln(embed_fold(embed_resample(mel, dt)), pw, pb, lnw, lnb)


def _bf16_np(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy()


def _np64(t):
    return t.to(torch.float64).numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def swin_qkv(x, n1w, n1b, wqkv, qkvb, rounded):
    """x [M, 96] -> LN1 (eps 1e-5) -> qkv [M, 288], float64 numpy"""
    x = _np64(x)
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    h = (x - mean) / np.sqrt(var + 1e-5) * _np64(n1w) + _np64(n1b)
    if rounded:
        h = _bf16_np(h)
    qkv = h @ _np64(wqkv).T + _np64(qkvb)
    return _bf16_np(qkv) if rounded else qkv


def swin_attention(qkv, relb, B, shift, rounded):
    """qkv [B*4096, 288] -> [B*4096, 96] in original token order: tests/swin_window_ref.window_attention, or (rounded) the
    same with the unnormalised softmax weights and the output rounded to bf16"""
    if not rounded:
        return sw.window_attention(qkv, _np64(relb), B, 64, 96, shift)
    q, k, v = sw.split_heads(sw.partition(_np64(qkv).reshape(B, 64, 64, 288), 64, shift), 96)
    att = q @ k.swapaxes(-1, -2) * sw.HEAD_DIM ** -0.5 + _np64(relb)[None, None]
    if shift:
        reg = sw.regions(64, shift)
        att = att + ((reg[:, None, :] != reg[:, :, None]) * -100.0)[None, :, None]
    p = np.exp(att - att.max(-1, keepdims=True))
    o = (_bf16_np(p) @ v) / p.sum(-1, keepdims=True)
    return _bf16_np(sw.merge(sw.join_heads(o), 64, shift).reshape(B * 4096, 96))


def swin_proj(x, o, wproj, pb):
    return _np64(x) + o @ _np64(wproj).T + _np64(pb)


def swin96_ref(x, n1w, n1b, wqkv, qkvb, relb, wproj, pb, B, shift, rounded):
    """[B*4096, 96] float64 torch"""
    o = swin_attention(swin_qkv(x, n1w, n1b, wqkv, qkvb, rounded), relb, B, shift, rounded)
    return torch.from_numpy(swin_proj(x, o, wproj, pb))


def merge_ln_ref(x, w, b):
    """x [B, H, H, C] -> [B*(H/2)^2, 4C]"""
    m = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], dim=-1)
    return layer_norm(m.reshape(-1, 4 * x.shape[-1]), w, b)


def latent_ref(x, nw, nb):
    """x [B, 64, 768] -> [B, 768]"""
    return layer_norm(x, nw, nb).mean(dim=1)


def proj_ln_norm_ref(e, lw, lb):
    y = layer_norm(e, lw, lb)
    return y / torch.sqrt((y * y).sum(dim=-1, keepdim=True))


def block1_conv1(mel, w0, s0, dt, mid_bf16=True):
    """mel [B, T, 64] -> relu(conv 1 + s0) [B, 64, T, 64] (channel, time, frequency), rounded to bf16 as the kernel keeps it"""
    y = F.relu(F.conv2d(mel.to(dt)[:, None], w0.to(dt).reshape(64, 1, 3, 3), padding=1) + s0.to(dt).view(1, 64, 1, 1))
    return y.to(torch.bfloat16).to(dt) if mid_bf16 else y


def block1_conv2(mid_padded, Wt, bias2):
    """mid [B, 64, T + 2, 66] WITH its padding border -> relu(conv 2 + bias2) [B, 64, T, 64]; Wt [64, 576], k = (kh*3 + kw)*64 + c"""
    dt = mid_padded.dtype
    w = Wt.to(dt).reshape(64, 3, 3, 64).permute(0, 3, 1, 2)
    return F.relu(F.conv2d(mid_padded, w) + bias2.to(dt).view(1, 64, 1, 1))


def block1_pool(y):
    """[B, 64, T, 64] -> 2x2 mean (floor) -> [B*(T/2)*32, 64], position-major"""
    p = F.avg_pool2d(y, kernel_size=2)
    return p.permute(0, 2, 3, 1).reshape(-1, 64)


def block1_ref(mel, w0, s0, Wt, bias2, dt, mid_bf16=True):
    return block1_pool(block1_conv2(F.pad(block1_conv1(mel, w0, s0, dt, mid_bf16), (1, 1, 1, 1)), Wt, bias2))


def head_pool_ref(x):
    """x [B, T, F, C] -> [B, C]"""
    m = x.mean(dim=2)
    return m.max(dim=1).values + m.mean(dim=1)


# ------------------------------------------------------------------------------------------------ guards and inputs
def nan_rows(rows, cols, dtype):
    t = torch.empty(rows, cols, dtype=dtype)
    if dtype == torch.bfloat16:
        t.view(torch.int16).fill_(BF16_GUARD)
    else:
        t.view(torch.int32).fill_(F32_GUARD)
    return t


def guarded(t, width=None):
    """a kernel input, flat: `t` and GUARD rows of NaN (rows of `width`, by default t's last dimension) behind it"""
    return torch.cat([t.reshape(-1), nan_rows(GUARD, width or t.shape[-1], t.dtype).reshape(-1)])


def out_buffer(rows, cols, dtype):
    """an output: [rows + GUARD, cols], all of it the NaN pattern (an element nobody writes fails too)"""
    return nan_rows(rows + GUARD, cols, dtype)


def as_output(want, dtype):
    """what a kernel that computes `want` exactly would leave in out_buffer (for the checker's own tests)"""
    want = want.reshape(-1, want.shape[-1])
    return torch.cat([want.to(torch.float32).to(dtype), nan_rows(GUARD, want.shape[1], dtype)], dim=0)


def guards_intact(full, rows):
    g = full[rows:]
    if full.dtype == torch.bfloat16:
        return bool((g.view(torch.int16) == BF16_GUARD).all())
    return bool((g.view(torch.int32) == F32_GUARD).all())


def _rows(g, n, W, const_row, outlier_row):
    """[n, W] fp32: rows of differing scale and offset, one constant row (variance 0), one row with a single 1e4 outlier"""
    scale = torch.exp(0.8 * torch.randn(n, 1, generator=g))
    x = torch.randn(n, W, generator=g) * scale + 2.0 * torch.randn(n, 1, generator=g)
    x[const_row, :] = 1.25
    x[outlier_row, W // 3] = 1e4
    return x


def _ln_affine(g, W):
    return 1 + 0.1 * torch.randn(W, generator=g), 0.1 * torch.randn(W, generator=g)


def hilo_stream(x, lo_off):
    """fp32 [n] -> (bf16 buffer: hi at 0, lo at lo_off, NaN in between, values hi + lo in float64 [n])"""
    n = x.numel()
    hi = x.to(torch.bfloat16)
    lo = (x - hi.to(torch.float32)).to(torch.bfloat16)
    buf = nan_rows(1, lo_off + n, torch.bfloat16).reshape(-1)
    buf[:n] = hi
    buf[lo_off:] = lo
    return buf, hi.to(torch.float64) + lo.to(torch.float64)


class Problem:
    """one case: `inputs` as the kernel takes them (CPU, guard rows included), the output's shape and type, the references"""

    def __init__(self, kernel, case):
        self.kernel, self.case, self.what = kernel, case, case_id(kernel, case)
        self.kind = KIND[kernel]
        self.raw, self.inputs, self.special = {}, {}, {}       # raw: the same tensors without guards, for restating
        self.want = self.ref32 = self.exact = self.table = None
        self.lo_off = 0
        self.out_dtype = torch.float32 if self.kind in ("f32", "swin") else torch.bfloat16

    @property
    def rows(self):
        return self.want.shape[0]

    @property
    def cols(self):
        return self.want.shape[1]


def _seed(kernel, c):
    h = 17
    for ch in case_id(kernel, {k: v for k, v in c.items() if k not in ("form", "grid", "chunk")}):
        h = (h * 131 + ord(ch)) % (2 ** 31 - 1)
    return h


def rel_bias(table):
    """[225, 4] table -> [4, 64, 64], the way pack_htsat_weights expands it"""
    return table[htsat_ref.rel_pos_index().reshape(-1)].reshape(64, 64, 4).permute(2, 0, 1).contiguous()


def build(kernel, c):
    """the inputs and references of one case; forms of a kernel that share a shape share the data"""
    g = torch.Generator().manual_seed(_seed(kernel, c))
    rn = lambda *s: torch.randn(*s, generator=g)
    p = Problem(kernel, c)
    if kernel == "embed":
        B, Fc = c["B"], c["Fc"]
        # log-mel + bn0: O(1) steps between neighbouring frames and bins on a slow trend, clips of different level
        mel = rn(B, Fc, 64) + 0.5 * torch.arange(B).view(B, 1, 1) + torch.sin(torch.arange(Fc) / 37.0).view(1, Fc, 1)
        pw, pb = 0.25 * rn(96, 16), 0.1 * rn(96)
        lnw, lnb = _ln_affine(g, 96)
        p.raw = dict(mel=mel, pw=pw, pb=pb, lnw=lnw, lnb=lnb)
        p.want = embed_ref(mel, pw, pb, lnw, lnb, torch.float64)
        p.ref32 = embed_ref(mel, pw, pb, lnw, lnb, torch.float32)
    elif kernel == "swin96":
        B, shift = c["B"], c["shift"]
        M = B * 4096
        const_row, outlier_row = M - 1, 10 * 64 + 20          # the last token of the last clip (a masked window); clip 0
        x = _rows(g, M, 96, const_row, outlier_row)
        n1w, n1b = _ln_affine(g, 96)
        wqkv, qkvb = (0.1 * rn(288, 96)).to(torch.bfloat16), 0.1 * rn(288)
        p.table = 0.5 * rn(225, 4)                            # a bias that is Toeplitz in (dy, dx): the kernel's contract
        relb = rel_bias(p.table)
        wproj, pb = (0.1 * rn(96, 96)).to(torch.bfloat16), 0.1 * rn(96)
        p.raw = dict(x=x, n1w=n1w, n1b=n1b, wqkv=wqkv, qkvb=qkvb, relb=relb, wproj=wproj, pb=pb)
        p.want = swin96_ref(x, n1w, n1b, wqkv, qkvb, relb, wproj, pb, B, shift, True)
        p.exact = swin96_ref(x, n1w, n1b, wqkv, qkvb, relb, wproj, pb, B, shift, False)
        p.special = {"constant row": const_row, "outlier row": outlier_row}
    elif kernel == "merge_ln":
        B, H, C = c["B"], c["H"], c["C"]
        n = B * H * H
        # the LayerNorm row is four tokens: tokens (0,0) (1,0) (0,1) (1,1) of the last clip constant, one outlier in clip 0
        x = _rows(g, n + 2, C, n + 1, n)[:n].reshape(B, H, H, C)
        x[0, 1, 0, C // 3] = 1e4
        x[B - 1, H - 2:, H - 2:, :] = 1.25
        w, b = _ln_affine(g, 4 * C)
        p.raw = dict(x=x, w=w, b=b)
        if c["hilo"]:
            p.lo_off = ceil128(n) * C
            buf, val = hilo_stream(x.reshape(-1), p.lo_off)
            p.raw["x"], p.raw["x_val"], p.raw["hi"] = buf, val.reshape(B, H, H, C), buf[:n * C].reshape(B, H, H, C)
            p.want = merge_ln_ref(val.reshape(B, H, H, C), w, b)
            p.ref32 = merge_ln_ref(val.reshape(B, H, H, C).to(torch.float32), w, b)
        else:
            p.want, p.ref32 = merge_ln_ref(x.double(), w, b), merge_ln_ref(x, w, b)
    elif kernel == "latent":
        B = c["B"]
        x = _rows(g, B * 64, 768, B * 64 - 1, 5)
        nw, nb = _ln_affine(g, 768)
        p.raw = dict(x=x, nw=nw, nb=nb)
        if c["hilo"]:
            p.lo_off = ceil128(B * 64) * 768
            buf, val = hilo_stream(x.reshape(-1), p.lo_off)
            p.raw["x"], p.raw["x_val"], p.raw["hi"] = buf, val.reshape(B, 64, 768), buf[:B * 64 * 768].reshape(B, 64, 768)
            p.want = latent_ref(val.reshape(B, 64, 768), nw, nb)
            p.ref32 = latent_ref(val.reshape(B, 64, 768).to(torch.float32), nw, nb)
        else:
            p.want, p.ref32 = latent_ref(x.double().reshape(B, 64, 768), nw, nb), latent_ref(x.reshape(B, 64, 768), nw, nb)
    elif kernel == "proj_ln_norm":
        B = c["B"]
        if B >= 4:
            e = _rows(g, B, 1024, B - 1, B - 2)
            e[0] *= 0.02 / e[0].std()                        # a row whose variance is near eps
        else:
            e = _rows(g, B + 2, 1024, B + 1, B)[:B]          # one row: neither
        lw, lb = _ln_affine(g, 1024)
        p.raw = dict(e=e, lw=lw, lb=lb)
        p.want, p.ref32 = proj_ln_norm_ref(e.double(), lw, lb), proj_ln_norm_ref(e, lw, lb)
    elif kernel == "block1":
        B, T = c["B"], c["T"]
        mel = rn(B, T, 64) + 0.5 * torch.arange(B).view(B, 1, 1) + torch.sin(torch.arange(T) / 11.0).view(1, T, 1)
        w0, s0 = rn(64, 9) / 3, 0.1 * rn(64)                  # conv 1 is symmetric about s0: ReLU cuts about half
        s0 = s0 - (w0.sum(1) * mel.mean())                    # ... whatever the level of the log-mel
        Wt, bias2 = (rn(64, 576) / 24).to(torch.bfloat16), 0.1 * rn(64)
        p.raw = dict(mel=mel, w0=w0, s0=s0, Wt=Wt, bias2=bias2)
        p.want = block1_ref(mel, w0, s0, Wt, bias2, torch.float64)
    else:
        assert kernel == "head_pool"
        B, T, Fq, C = c["B"], c["T"], c["F"], c["C"]
        x = (rn(B, T, Fq, C).abs() * torch.exp(0.5 * rn(B, T, 1, 1)) + 0.3 * rn(1, 1, 1, C)).to(torch.bfloat16)
        p.raw = dict(x=x)
        p.want, p.ref32 = head_pool_ref(x.double()), head_pool_ref(x.float())
    for k, v in p.raw.items():
        if k not in ("x_val", "hi"):
            p.inputs[k] = guarded(v, p.raw["hi"].shape[-1] if (k == "x" and p.lo_off) else None)
    return p


# ------------------------------------------------------------------------------------------------ the checker
def where(bad, what):
    idx = bad.nonzero()
    r, c = (int(v) for v in idx[0])
    return f"{what}: {idx.shape[0]} of {bad.numel()} elements are off, the first at row {r}, column {c}"


def row_tau(want, ref32):
    """per output row: max(8 x the float32 restatement's own error, 16 fp32 steps at the row's scale)"""
    err = (ref32.double() - want).abs().amax(dim=1, keepdim=True)
    return torch.maximum(8 * err, 2.0 ** -20 * want.abs().amax(dim=1, keepdim=True))


def flip_share(got, want):
    """the share of elements that are not bf16(want)"""
    return float((got.to(torch.float32) != want.to(torch.float32).to(torch.bfloat16).to(torch.float32)).double().mean())


def swin_ratios(got, want, exact, special):
    """{group: (max |got - rounded| / max n, mean |got - rounded| / mean n, the group's rows, its max n)} with
    n = |rounded - exact|: all rows but the special ones together, each special row by itself"""
    d, n = (got.double() - want).abs(), (want - exact).abs()
    rest = torch.ones(want.shape[0], dtype=torch.bool)
    rest[list(special.values())] = False
    out = {}
    for name, sel in [("rows", rest)] + [(f"{k} {r}", torch.tensor([r])) for k, r in special.items()]:
        out[name] = (float(d[sel].max() / n[sel].max()), float(d[sel].mean() / n[sel].mean()), sel, float(n[sel].max()))
    return out


def check(p, full):
    """`full` [rows + GUARD, cols]: what came back in out_buffer (swin96: in the guarded x).  Raises AssertionError naming the
    case, the first bad row and column and the number of bad elements; returns the figures it printed."""
    what, rows = p.what, p.rows
    assert full.dtype == p.out_dtype and tuple(full.shape) == (rows + GUARD, p.cols), f"{what}: buffer {tuple(full.shape)} {full.dtype}"
    assert guards_intact(full, rows), f"{what}: guard rows written"
    got = full[:rows]
    finite = torch.isfinite(got.to(torch.float32))
    assert bool(finite.all()), where(~finite, what + " (not finite)")
    got64, want, fig = got.to(torch.float64), p.want, {}
    if p.kind == "f32":
        err, tau = (got64 - want).abs(), row_tau(want, p.ref32)
        fig["max err / tau"] = float((err / tau).max())
        print(f"{what}: max |got - want64| / tau_r = {fig['max err / tau']:.3f}")
        assert bool((err <= tau).all()), where(~(err <= tau), what)
    elif p.kind == "bf16":
        err = (got64 - want).abs()
        tol = 2.0 ** -8 * want.abs() + row_tau(want, p.ref32)
        fig["max err / bound"], fig["flips"] = float((err / tol).max()), flip_share(got, want)
        print(f"{what}: max |got - want64| / bound = {fig['max err / bound']:.3f}, {100 * fig['flips']:.4f} % are not bf16(want64)")
        assert bool((err <= tol).all()), where(~(err <= tol), what)
        assert fig["flips"] <= 0.01, f"{what}: {100 * fig['flips']:.2f} % of the elements are not bf16(want64) (at most 1 %)"
    elif p.kind == "swin":
        ratios = swin_ratios(got, want, p.exact, p.special)
        for name, (rmax, rmean, sel, nmax) in ratios.items():
            fig[name] = (rmax, rmean)
            print(f"{what} {name}: max |got - rounded| / max n = {rmax:.3f}, mean |got - rounded| / mean n = {rmean:.3f}")
        for name, (rmax, rmean, sel, nmax) in ratios.items():
            bad = torch.zeros_like(want, dtype=torch.bool)
            bad[sel] = (got64 - want).abs()[sel] > 2 * nmax
            assert not bool(bad.any()), where(bad, f"{what} {name} (beyond 2 max n = {2 * nmax:.3e})")
            assert rmean <= 2, f"{what} {name}: mean |got - rounded| is {rmean:.3f} x mean n (at most 2)"
    else:
        err = (got64 - want).abs()
        tol = 2e-3 + 8e-3 * want.abs()
        fig["max err / bound"] = float((err / tol).max())
        print(f"{what}: max |got - want64| / (2e-3 + 8e-3 |want64|) = {fig['max err / bound']:.3f}")
        assert bool((err <= tol).all()), where(~(err <= tol), what)
    return fig

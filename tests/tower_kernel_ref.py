"""The image and text towers' own kernels (csrc/vit.hip, csrc/text.hip, csrc/xlmr_text.hip), one by one: the case table, a float64
restatement of each operation with the same expression in float32, seeded inputs, and the checker.  Plain torch on the CPU:
tests/test_gpu_tower_kernels.py runs the kernels against it through the wise_debug_* twins (the LayerNorm family through the
product's wise_layernorm_f32_bf16), tests/test_tower_kernel_ref_cpu.py holds the table, the restatements (against oracle/vit_ref.py,
siglip_ref.py, text_ref.py, xlmr_text_ref.py, clap_bert_ref.py) and the checker (against planted faults) to account without a GPU.
Guards, NaN patterns, row_tau, flip_share and where are tests/audio_kernel_ref.py's.

Restatements state the operation as the oracles do, not the kernel's code:

  patchify      ToTensor + Normalize of a u8 frame in float32 with two true divisions (vit_ref.normalize_u8; mean = std = 0.5 for
                the SigLIP towers), the gather k = c P P + py P + px (vit_ref.patchify), rounded to bf16, zero columns up to Kp
  embed_pos     patch rows + pos[row % T]                              (siglip_ref.siglip_vision_forward)
  embed_lnpre   LayerNorm(cat(cls, patch rows) + pos), eps 1e-5        (vit_ref.vit_forward's first tap); the fold form splits the
                row into bf16 hi + lo and adds rstd of the NORMALISED row (the scale the first folded GEMM takes)
  cls_ln        LayerNorm of one row per sequence: row 0, or row pos[b]
  l2norm_rows   e / ||e||, no epsilon
  map_pool      per head softmax(q k^T / 8) v with one latent query    (siglip_ref._attention)
  hilo_rows     hi + lo of selected rows of a bf16 hi + lo stream
  layernorm     (x - mean) / sqrt(var + eps) * w + b; the dual form also returns the fp32 rows
  text_embed    tok_emb[ids] + pos_emb[t]; the pooled position: first argmax of the ids | ne(ids, 0).sum - 1 | T - 1
  xlmr_embed    (word[ids] + pos[p]) + type0 with p = cumsum(mask) mask + pad (RoBERTa) | arange(T) (BERT); lens = sum(mask)
  xlmr_meanpool sum of the first lens rows / lens | row 0

An output is one of four kinds.  `bits`: equal to the expectation bit for bit (torch.equal on the bit patterns: one rounded fp32
operation in the kernel is one in torch; integers).  `f32`: |got - want64| <= row_tau, which is 8 x the float32 restatement's own
error per row and at least 16 fp32 steps at the row's scale.  `bf16`: <= 2^-8 |want64| + row_tau, and at most 1 % of the elements
may differ from bf16(want64).  `lo`: hi + lo within row_tau + 2^-16 |want64| of want64 (lo = bf16(n - hi) is off by up to 2^-9 of
half a bf16 step of n, 2^-18 |n|) and |lo| <= 2^-8 |hi|: hi is n ROUNDED to bf16.  Every buffer a kernel writes is prefilled with
the NaN pattern and has GUARD rows behind it; rows the kernel must leave alone (the gap between hi and lo, the rows between two
strided rows) are expected to hold the pattern still."""
import torch

from oracle import vit_ref
from tests import audio_kernel_ref as ak
from tests.audio_kernel_ref import GUARD, flip_share, guarded, guards_intact, layer_norm, nan_rows, out_buffer, row_tau, where
from tests.test_gpu_row_kernel_hashes import LN_SHAPES

F64, F32, BF16, I32 = torch.float64, torch.float32, torch.bfloat16, torch.int32
VOCAB = 64
BT = ((1, 1), (3, 5), (2, 64), (2, 65), (3, 77), (2, 128))       # B*T % 4 != 0: the last workgroup of four waves is ragged
PATCH_SHAPES = ((2, 16, 8, 0), (2, 28, 14, 0), (2, 32, 16, 0), (2, 32, 16, 4))      # B, S, P, byte offset of the input pointer

# ------------------------------------------------------------------------------------------------ the case table
CASES = {
    "patchify": [dict(inp=i, arch=a, B=b, S=s, P=p, off=o) for i, archs in (("f32", (0,)), ("u8", (0, 1))) for a in archs
                 for b, s, p, o in PATCH_SHAPES],
    "embed_pos": [dict(B=b, T=t, W=w) for b, t in ((1, 1), (3, 5), (2, 65)) for w in (128, 384)],
    "embed_lnpre": [dict(fold=0, B=3, T=5, W=w) for w in (768, 1024, 1280, 1664, 2048)] + [dict(fold=1, B=3, T=5, W=768)],
    "cls_ln": [dict(pos=p, B=b, T=t, W=w) for w in (128, 512, 768, 1280, 2048) for p in (0, 1) for t in (1, 5, 77) for b in (1, 4, 5)],
    "l2norm": [dict(rows=r, D=d) for d in (4, 64, 100, 512, 1024) for r in (1, 4, 7)],
    "map_pool": [dict(data="random", B=2, T=t, W=128) for t in (1, 63, 64, 65, 196, 729, 1024)] +
                [dict(data="dominant", B=2, T=65, W=128), dict(data="equal", B=2, T=729, W=128)],
    "hilo_rows": [dict(n=n, stride=s, ostride=o, W=w) for n, s, o, w in ((3, 1, 1, 768), (3, 5, 1, 768), (3, 1, 5, 768), (7, 3, 2, 100))],
    "layernorm": [dict(rows=r, W=w) for r, w in LN_SHAPES],
    "layernorm_dual": [dict(inplace=i, eps=e, rows=7, W=w) for w in (132, 256, 768, 1024, 4096) for e in (1e-5, 1e-6, 1e-12) for i in (1, 0)],
    "text_embed": [dict(pool=p, B=b, T=t, W=w) for p in (0, 1, 2) for b, t in BT for w in (128, 384)],
    "xlmr_embed": [dict(pos_abs=a, pad=pad, B=b, T=t, W=w) for a in (0, 1) for pad in (1, 0) for b, t in BT for w in (256, 384)],
    "xlmr_meanpool": [dict(first=f, B=4, T=t, W=w) for f in (0, 1) for t in (77, 128) for w in (256, 1280)],
}
# kernel names as the sources define them (the ledger of tests/test_tower_kernel_ref_cpu.py)
KERNELS = {
    "patchify": ("patchify_kernel", "patchify8_kernel"), "embed_pos": ("embed_pos_kernel",), "embed_lnpre": ("embed_lnpre_kernel",),
    "cls_ln": ("cls_ln_kernel",), "l2norm": ("l2norm_rows_kernel",), "map_pool": ("map_pool_kernel",), "hilo_rows": ("hilo_rows_kernel",),
    "layernorm": ("layernorm_narrow_kernel", "layernorm_kernel", "layernorm_rows_kernel"), "layernorm_dual": ("layernorm_kernel",),
    "text_embed": ("text_embed_kernel",), "xlmr_embed": ("xlmr_embed_kernel",), "xlmr_meanpool": ("xlmr_meanpool_kernel",),
}


def case_id(kernel, c):
    return ak.case_id(kernel, c)


def kpad(P):
    """vit_dims / VitSpec.kpad: 3 P P rounded up to 64"""
    return (3 * P * P + 63) // 64 * 64


def patchify_form(c):
    """the kernel launch_patchify picks (vit_forward_part's fast_gather rule)"""
    fast = c["P"] % 8 == 0 and c["S"] % 8 == 0 and kpad(c["P"]) == 3 * c["P"] ** 2 and c["off"] % 16 == 0
    return ("patchify8_kernel" if fast else "patchify_kernel") + ("<u8>" if c["inp"] == "u8" else "<float>")


def layernorm_form(rows, W):
    """the kernel layernorm_f32_bf16 picks"""
    nv = (W // 4 + 63) // 64
    return "layernorm_narrow_kernel" if W <= 128 else (f"layernorm_rows_kernel<{nv},4>" if nv <= 2 and rows >= 16384 else f"layernorm_kernel<{nv}>")


# ------------------------------------------------------------------------------------------------ restatements
SIGLIP_MEAN = SIGLIP_STD = (0.5, 0.5, 0.5)


def normalize_u8(frames, arch, dt=F32, reciprocal=False):
    """ToTensor's division by 255, then Normalize's subtraction and division (vit_ref.normalize_u8 for arch 0)"""
    mean, std = (vit_ref.CLIP_MEAN, vit_ref.CLIP_STD) if arch == 0 else (SIGLIP_MEAN, SIGLIP_STD)
    mean, std = (torch.tensor(v, dtype=F32).to(dt).view(1, 3, 1, 1) for v in (mean, std))
    if reciprocal:       # the planted fault: x * (1 / 255) and * (1 / std)
        return (frames.to(dt) * (torch.ones((), dtype=dt) / 255.0) - mean) * (1.0 / std)
    return (frames.to(dt) / 255.0 - mean) / std


def patch_rows(x, P):
    """[B, 3, S, S] -> [B g g, Kp], k = c P P + py P + px, zero from K on"""
    p = vit_ref.patchify(x, P).reshape(-1, 3 * P * P)
    return torch.cat([p, torch.zeros(p.shape[0], kpad(P) - p.shape[1], dtype=p.dtype)], dim=1)


def embed_lnpre_ref(patch, cls, pos, w, b, B, T, eps=1e-5):
    """[B (T-1), W], [W], [T, W] -> the normalised rows [B T, W] (and the rows in front of the LayerNorm)"""
    W = cls.shape[0]
    x = torch.cat([cls.view(1, 1, W).expand(B, 1, W), patch.reshape(B, T - 1, W)], dim=1) + pos
    return layer_norm(x, w, b, eps).reshape(B * T, W), x.reshape(B * T, W)


def row_rstd(n, eps=1e-5):
    """LnRow::restat: rstd of the rows as they stand"""
    mean = n.mean(dim=-1, keepdim=True)
    return 1 / torch.sqrt(((n - mean) ** 2).mean(dim=-1, keepdim=True) + eps)


def l2norm_ref(e):
    return e / torch.sqrt((e * e).sum(dim=-1, keepdim=True))


def map_pool_ref(kv, qv, B, T, W, skip_last_slice=False):
    """kv [B T, 2W] (keys | values), qv [W] -> [B, W]: siglip_ref._attention with one query, head dim 64"""
    dt, H = kv.dtype, W // 64
    k = kv[:, :W].reshape(B, T, H, 64).transpose(1, 2)
    v = kv[:, W:].reshape(B, T, H, 64).transpose(1, 2)
    if skip_last_slice:      # the planted fault: tokens from 64 ((T - 1) // 64) on never enter
        n = (T - 1) // 64 * 64
        k, v = k[:, :, :n], v[:, :, :n]
    q = qv.to(dt).reshape(1, H, 1, 64)
    s = (q @ k.transpose(-1, -2)) / 8.0
    s = s - s.max(dim=-1, keepdim=True).values
    e = torch.exp(s)
    return ((e / e.sum(dim=-1, keepdim=True)) @ v).transpose(1, 2).reshape(B, W)


def text_pool_pos(ids, pool):
    ids = ids.to(torch.int64)
    T = ids.shape[1]
    if pool == 0:
        return ids.argmax(dim=-1)
    if pool == 1:
        return (torch.ne(ids, 0).sum(-1) - 1) % T            # torch indexes -1 from the end
    return torch.full((ids.shape[0],), T - 1)


def xlmr_positions(ids, pad, pos_abs):
    ids = ids.to(torch.int64)
    mask = (ids != pad).to(torch.int64)
    if pos_abs:
        return torch.arange(ids.shape[1]).expand_as(ids), mask.sum(-1)
    return torch.cumsum(mask, dim=1) * mask + pad, mask.sum(-1)


def meanpool_ref(x, lens, over_T=False):
    """x [B, T, W] -> [B, W]: the mean of the first lens[b] rows (over_T: the planted fault, the sum still over lens rows)"""
    out = torch.stack([x[b, :int(n)].sum(dim=0) / (x.shape[1] if over_T else int(n)) for b, n in enumerate(lens)])
    return out


# ------------------------------------------------------------------------------------------------ problems
class Out:
    """one buffer a kernel writes: [rows + GUARD, cols] of `dtype`.  want: float64 (f32 / bf16 / lo) or the exact tensor (bits);
    keep: bool [rows] — rows the kernel must leave as the pattern"""

    def __init__(self, kind, want, ref32=None, dtype=None, keep=None, hi=None):
        self.kind, self.want, self.ref32, self.keep, self.hi = kind, want, ref32, keep, hi
        self.dtype = dtype or (want.dtype if kind == "bits" else {"f32": F32, "bf16": BF16, "lo": BF16}[kind])
        self.rows, self.cols = want.shape


class Problem:
    def __init__(self, kernel, case):
        self.kernel, self.case, self.what = kernel, case, case_id(kernel, case)
        self.raw, self.inputs, self.outs, self.args = {}, {}, {}, {}


def _seed(kernel, c, drop=("off", "inplace", "fold", "first")):
    h = 29
    for ch in case_id(kernel, {k: v for k, v in c.items() if k not in drop}):
        h = (h * 131 + ord(ch)) % (2 ** 31 - 1)
    return h


def _int_rows(v):
    return v.to(I32).reshape(-1, 1)


def _tokens_text(g, c):
    """ids in [1, 62] with the pooling patterns planted; returns (ids [B, T] int32, what each row plants)"""
    B, T, pool = c["B"], c["T"], c["pool"]
    ids = torch.randint(1, VOCAB - 1, (B, T), generator=g)
    plants = []
    for b in range(B):
        if pool == 0:
            options = ["only slot"] if T == 1 else (["same lane", "adjacent", "last slot"] if T > 64 else ["adjacent", "last slot", "first slot"])
            plant = options[b % len(options)]
            t = (3 * b + 1) % max(1, T - 64)
            at = {"same lane": (t, t + 64), "adjacent": (T // 2, T // 2 + 1) if T > 2 else (0, 1), "last slot": (T - 1,),
                  "first slot": (0,), "only slot": (0,)}[plant]
            ids[b, list(at)] = VOCAB - 1
            free = [t for t in range(T) if t not in at]
        else:
            # right-padded with id 0; one zero inside the text too (the count is not the last non-zero index)
            plant = ("partial", "all zero", "full")[(b + T) % 3] if pool == 1 else "any"
            n = {"partial": T // 2 + 1, "all zero": 0, "full": T, "any": max(1, T - b)}[plant]
            ids[b, n:] = 0
            free = list(range(1, n - 1))
            if free:
                ids[b, free[-1]] = VOCAB - 1
                free = free[:-1]
        if free:
            ids[b, free[len(free) // 2]] = 0
        plants.append(plant)
    return ids.to(I32), plants


def xlmr_lens(c):
    """token counts of the rows: 1, 2, T - 1 and T by turns"""
    T = c["T"]
    options = [1, 2, T - 1, T]
    off = BT.index((c["B"], T)) + 2 * c["pos_abs"] + c["pad"]
    return [min(T, max(1, options[(b + off) % 4])) for b in range(c["B"])]


def build(kernel, c):
    """the inputs and expectations of one case; forms of a kernel that share a shape share the data"""
    g = torch.Generator().manual_seed(_seed(kernel, c))
    rn = lambda *s: torch.randn(*s, generator=g)
    p = Problem(kernel, c)
    if kernel == "patchify":
        B, S, P = c["B"], c["S"], c["P"]
        if c["inp"] == "u8":     # every byte value in every channel of every frame (S S >= 256)
            img = torch.stack([torch.randperm(S * S, generator=g) % 256 for _ in range(B * 3)]).reshape(B, 3, S, S).to(torch.uint8)
            x32, x64 = normalize_u8(img, c["arch"]), normalize_u8(img, c["arch"], F64)
            p.raw["x64"] = patch_rows(x64, P)
        else:
            img = rn(B, 3, S, S) * torch.exp(rn(B, 3, 1, 1))
            x32 = img
        p.raw["img"] = img
        p.outs["patches"] = Out("bits", patch_rows(x32, P).to(BF16))
        pad = torch.full((c["off"],), 0xA5, dtype=torch.uint8)
        tail = nan_rows(GUARD, S, F32).reshape(-1).view(torch.uint8) if c["inp"] == "f32" else torch.full((GUARD * S,), 0xA5, dtype=torch.uint8)
        p.inputs["img"] = torch.cat([pad, img.reshape(-1).view(torch.uint8), tail])           # the kernel's pointer is base + off
    elif kernel == "embed_pos":
        B, T, W = c["B"], c["T"], c["W"]
        patch, pos = rn(B * T, W) * 3, rn(T, W) * 0.25 + torch.arange(T).view(T, 1)
        p.raw = dict(patch=patch, pos=pos)
        p.outs["x"] = Out("bits", (patch.reshape(B, T, W) + pos).reshape(B * T, W))
    elif kernel == "embed_lnpre":
        B, T, W = c["B"], c["T"], c["W"]
        # cls, pos rows and patch rows of clearly different scale and level: a row taken one off moves every element
        patch = rn(B * (T - 1), W) * torch.exp(0.8 * rn(B * (T - 1), 1)) + 2.0 * rn(B * (T - 1), 1)
        cls, pos = 4.0 * rn(W), 0.5 * rn(T, W) * (1 + torch.arange(T).view(T, 1))
        w, b = ak._ln_affine(g, W)
        p.raw = dict(patch=patch, cls=cls, pos=pos, w=w, b=b)
        want, _ = embed_lnpre_ref(patch.double(), cls.double(), pos.double(), w, b, B, T)
        ref32, _ = embed_lnpre_ref(patch, cls, pos, w, b, B, T)
        rows = B * T
        if c["fold"]:
            p.args["lo_rows"] = ak.ceil128(rows)             # lo starts this many rows behind hi: the gap stays the pattern
            gap = p.args["lo_rows"] - rows
            keep = torch.cat([torch.zeros(rows, dtype=torch.bool), torch.ones(gap, dtype=torch.bool), torch.zeros(rows, dtype=torch.bool)])
            pad = torch.zeros(gap, W, dtype=F64)
            p.outs["hilo"] = Out("lo", torch.cat([want, pad, want]), torch.cat([ref32, pad.float(), ref32]), keep=keep)
            p.outs["rstd"] = Out("f32", row_rstd(want), row_rstd(ref32))
        else:
            p.outs["x"] = Out("f32", want, ref32)
    elif kernel == "cls_ln":
        B, T, W = c["B"], c["T"], c["W"]
        pos = torch.tensor([(0, T - 1, T // 2)[b % 3] for b in range(B)]) if c["pos"] else torch.zeros(B, dtype=torch.int64)
        row = torch.arange(B) * T + pos
        x = ak._rows(g, B * T + 2, W, B * T, B * T + 1)[:B * T]
        if B >= 4:               # the pooled rows of the last two sequences: one constant, one with a single outlier
            x[row[B - 1]] = 1.25
            x[row[B - 2], W // 3] = 1e4
        w, b = ak._ln_affine(g, W)
        p.raw = dict(x=x, w=w, b=b)
        if c["pos"]:
            p.raw["pos"] = pos.to(I32)
        p.args["row"] = row
        p.outs["y"] = Out("bf16", layer_norm(x.double()[row], w, b), layer_norm(x[row], w, b))
    elif kernel == "l2norm":
        rows, D = c["rows"], c["D"]
        e = rn(rows, D) * torch.tensor([(1e-3, 1.0, 1e3)[r % 3] for r in range(rows)]).view(rows, 1)
        p.raw = dict(e=e)
        p.outs["out"] = Out("f32", l2norm_ref(e.double()), l2norm_ref(e))
    elif kernel == "map_pool":
        B, T, W = c["B"], c["T"], c["W"]
        qv = 2.0 * rn(W)
        kv = rn(B * T, 2 * W)
        if c["data"] == "dominant":          # key T - 1 of every frame = q: its score is |q_h|^2 / 8, about 32; the rest lie in +-10
            kv.reshape(B, T, 2 * W)[:, T - 1, :W] = qv
        elif c["data"] == "equal":           # one key for every token: every score equal, the output is the mean of V
            kv.reshape(B, T, 2 * W)[:, :, :W] = rn(1, 1, W)
        kv = kv.to(BF16)
        p.raw = dict(kv=kv, qv=qv)
        p.outs["o"] = Out("bf16", map_pool_ref(kv.double(), qv, B, T, W), map_pool_ref(kv.float(), qv, B, T, W))
    elif kernel == "hilo_rows":
        n, stride, ostride, W = c["n"], c["stride"], c["ostride"], c["W"]
        rows_in, rows_out = (n - 1) * stride + 1, (n - 1) * ostride + 1
        x = rn(rows_in, W) * torch.exp(rn(rows_in, 1))
        p.args["lo_off"] = ak.ceil128(rows_in) * W
        buf, _ = ak.hilo_stream(x.reshape(-1), p.args["lo_off"])
        p.raw = dict(hi=buf)
        hi, lo = buf[:rows_in * W].reshape(rows_in, W), buf[p.args["lo_off"]:].reshape(rows_in, W)
        want = nan_rows(rows_out, W, F32)
        want[::ostride] = (hi.float() + lo.float())[::stride]
        keep = torch.ones(rows_out, dtype=torch.bool)
        keep[::ostride] = False
        p.outs["out"] = Out("bits", want, keep=keep)
    elif kernel == "layernorm":
        rows, W = c["rows"], c["W"]      # tests/test_gpu_row_kernel_hashes.py's recipe
        g = torch.Generator().manual_seed(rows * 8192 + W)
        x = torch.randn(rows, W, generator=g) * 3 + 0.5
        w = 1 + 0.1 * torch.randn(W, generator=g)
        b = 0.1 * torch.randn(W, generator=g)
        x[rows - 1, :] = 1.25
        x[rows - 2, W // 3] = 1e4
        p.raw = dict(x=x, w=w, b=b)
        p.outs["y"] = Out("bf16", layer_norm(x.double(), w, b), layer_norm(x, w, b))
    elif kernel == "layernorm_dual":
        rows, W, eps = c["rows"], c["W"], c["eps"]
        x = ak._rows(g, rows, W, rows - 1, rows - 2)
        if eps < 1e-9:       # rstd = 1e6 would turn the rounding noise of a constant row's input into the answer: tiny variance instead
            x[rows - 1] = 1.25 + 2.0 ** -12 * (2.0 * torch.randint(0, 2, (W,), generator=g) - 1)
        w, b = ak._ln_affine(g, W)
        p.raw = dict(x=x, w=w, b=b)
        want, ref32 = layer_norm(x.double(), w, b, eps), layer_norm(x, w, b, eps)
        p.outs["xo"] = Out("f32", want, ref32)
        p.outs["y"] = Out("bf16", want, ref32)
    elif kernel == "text_embed":
        B, T, W = c["B"], c["T"], c["W"]
        ids, p.args["plants"] = _tokens_text(g, c)
        tok, pos = 0.5 * rn(VOCAB, W), 0.25 * rn(T, W)
        p.raw = dict(ids=ids, tok=tok, pos=pos)
        p.outs["x"] = Out("bits", (tok[ids.long()] + pos).reshape(B * T, W))
        p.outs["eot"] = Out("bits", _int_rows(text_pool_pos(ids, c["pool"])))
    elif kernel == "xlmr_embed":
        B, T, W, pad = c["B"], c["T"], c["W"], c["pad"]
        lens = xlmr_lens(c)
        ids = torch.randint(2, VOCAB - 1, (B, T), generator=g)
        for b, n in enumerate(lens):
            ids[b, n:] = pad
            if n > 2:
                ids[b, n // 2], ids[b, 0] = VOCAB - 1, (0 if pad else ids[b, 0])
        ids = ids.to(I32)
        p.args.update(lens=lens, max_pos=T + pad + 2)
        word, pos, type0 = 0.5 * rn(VOCAB, W), 0.25 * rn(p.args["max_pos"], W) + torch.arange(p.args["max_pos"]).view(-1, 1), 0.1 * rn(W)
        p.raw = dict(ids=ids, word=word, pos=pos, type0=type0)
        pid, n = xlmr_positions(ids, pad, c["pos_abs"])
        p.args["pid"] = pid
        p.outs["x"] = Out("bits", ((word[ids.long()] + pos[pid]) + type0).reshape(B * T, W))
        p.outs["lens"] = Out("bits", _int_rows(n))
    else:
        assert kernel == "xlmr_meanpool"
        B, T, W = c["B"], c["T"], c["W"]
        lens = [1, 2, T - 1, T]
        x = rn(B, T, W) + 0.5 * rn(B, 1, W)
        for b, n in enumerate(lens):         # rows past the length: a read there shows as NaN
            x[b, n:] = nan_rows(T - n, W, F32)
        p.raw = dict(x=x, lens=torch.tensor(lens, dtype=I32))
        if c["first"]:
            p.outs["pooled"] = Out("bits", x[:, 0].to(BF16))
        else:
            p.outs["pooled"] = Out("bf16", meanpool_ref(x.double(), lens), meanpool_ref(x, lens))
    for k, v in p.raw.items():
        if k in p.inputs or k == "x64":
            continue
        if v.dtype in (F32, BF16):
            p.inputs[k] = guarded(v, c["W"] if k == "hi" else None)
        else:                # ids / lens / pos: four more integers
            p.inputs[k] = torch.cat([v.reshape(-1), torch.full((GUARD,), -1, dtype=v.dtype)])
    return p


# ------------------------------------------------------------------------------------------------ the checker
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def as_output(o, want=None):
    """what a kernel that computes `want` (default: the expectation itself) exactly would leave in the output's buffer"""
    want = o.want if want is None else want
    if o.kind == "bits" and want.dtype == o.dtype:
        body = want.clone()
    else:
        body = want.to(F32).to(o.dtype)
    if o.kind == "lo":       # hi rows, the gap, lo rows: split the first block
        n = int((~o.keep).sum()) // 2
        hi = want[:n].to(F32).to(BF16)
        body[:n], body[-n:] = hi, (want[:n] - hi.double()).to(F32).to(BF16)
    if o.keep is not None:
        body[o.keep] = nan_rows(int(o.keep.sum()), o.cols, o.dtype)
    return torch.cat([body, nan_rows(GUARD, o.cols, o.dtype)], dim=0)


def check(p, name, full):
    """`full` [rows + GUARD, cols]: what came back in the buffer of output `name`.  Raises AssertionError naming the case, the
    first bad row and column and the number of bad elements; returns the figures it printed."""
    o, what = p.outs[name], f"{p.what} {name}"
    assert full.dtype == o.dtype and tuple(full.shape) == (o.rows + GUARD, o.cols), f"{what}: buffer {tuple(full.shape)} {full.dtype}"
    assert guards_intact(full, o.rows), f"{what}: guard rows written"
    got, fig = full[:o.rows], {}
    live = torch.ones(o.rows, dtype=torch.bool) if o.keep is None else ~o.keep
    if o.keep is not None and bool(o.keep.any()):
        kept = _bits(got[o.keep]) == _bits(nan_rows(1, o.cols, o.dtype))
        assert bool(kept.all()), where(~kept, what + " (rows the kernel must leave alone)")
    if o.kind == "bits":
        bad = torch.zeros(o.rows, o.cols, dtype=torch.bool)
        bad[live] = _bits(got[live]) != _bits(o.want[live])
        fig["mismatches"] = int(bad.sum())
        print(f"{what}: {fig['mismatches']} of {bad.numel()} elements differ from the expected bits")
        assert not bool(bad.any()), where(bad, what)
        return fig
    finite = torch.isfinite(got.to(F32)) | ~live.view(-1, 1)
    assert bool(finite.all()), where(~finite, what + " (not finite)")
    got64, want = got.to(F64), o.want
    tau = row_tau(want, o.ref32)
    if o.kind == "f32":
        err = (got64 - want).abs()
        fig["max err / tau"] = float((err / tau).max())
        print(f"{what}: max |got - want64| / tau_r = {fig['max err / tau']:.3f}")
        assert bool((err <= tau).all()), where(~(err <= tau), what)
    elif o.kind == "bf16":
        err, tol = (got64 - want).abs(), 2.0 ** -8 * want.abs() + tau
        fig["max err / bound"], fig["flips"] = float((err / tol).max()), flip_share(got, want)
        print(f"{what}: max |got - want64| / bound = {fig['max err / bound']:.3f}, {100 * fig['flips']:.4f} % are not bf16(want64)")
        assert bool((err <= tol).all()), where(~(err <= tol), what)
        assert fig["flips"] <= 0.01, f"{what}: {100 * fig['flips']:.2f} % of the elements are not bf16(want64) (at most 1 %)"
    else:
        n = int(live.sum()) // 2
        hi, lo, w, t = got64[:n], got64[-n:], want[:n], tau[:n]
        assert bool(torch.isfinite(lo).all()), where(~torch.isfinite(lo), what + " (lo not finite)")
        err, tol = (hi - w).abs(), 2.0 ** -8 * w.abs() + t
        fig["hi: max err / bound"], fig["hi: flips"] = float((err / tol).max()), flip_share(got[:n], w)
        assert bool((err <= tol).all()), where(~(err <= tol), what + " (hi)")
        assert fig["hi: flips"] <= 0.01, f"{what}: {100 * fig['hi: flips']:.2f} % of hi are not bf16(want64) (at most 1 %)"
        err, tol = (hi + lo - w).abs(), t + 2.0 ** -16 * w.abs()
        fig["hi + lo: max err / bound"] = float((err / tol).max())
        assert bool((err <= tol).all()), where(~(err <= tol), what + " (hi + lo)")
        small = lo.abs() <= 2.0 ** -8 * hi.abs()
        assert bool(small.all()), where(~small, what + " (|lo| beyond half a step of hi)")
        print(f"{what}: hi max |got - want64| / bound = {fig['hi: max err / bound']:.3f}, {100 * fig['hi: flips']:.4f} % are not "
              f"bf16(want64); hi + lo max err / bound = {fig['hi + lo: max err / bound']:.3f}")
    return fig

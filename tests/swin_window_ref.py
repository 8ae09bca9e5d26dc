"""The window layout of HTSAT's shifted-window attention (msclap HTSAT WindowAttention / SwinTransformerBlock), stated once in
numpy float64: the cyclic shift, the partition into 8 x 8 windows, the shift regions and the attention itself.  Shared by
tests/test_gpu_swin_stream.py (a float64 reference on ordinary data) and tests/attention_exact_cases.py (exact data built in
window order and carried to the original token order through `merge`)."""
import numpy as np

WIN = 8
HEAD_DIM = 24


def partition(x, H, shift):
    """x [B, H, H, F] in original token order -> [B, windows, 64, F]: rolled by -shift, cut into 8 x 8 windows"""
    if shift:
        x = np.roll(x, shift=(-shift, -shift), axis=(1, 2))
    B, F, nw = x.shape[0], x.shape[-1], H // WIN
    return x.reshape(B, nw, WIN, nw, WIN, F).transpose(0, 1, 3, 2, 4, 5).reshape(B, nw * nw, WIN * WIN, F)


def merge(w, H, shift):
    """the inverse of partition: [B, windows, 64, F] -> [B, H, H, F] in original token order"""
    B, F, nw = w.shape[0], w.shape[-1], H // WIN
    x = w.reshape(B, nw, nw, WIN, WIN, F).transpose(0, 1, 3, 2, 4, 5).reshape(B, H, H, F)
    if shift:
        x = np.roll(x, shift=(shift, shift), axis=(1, 2))
    return x


def regions(H, shift):
    """[windows, 64]: the shift region (0..8) of every token of every window, in rolled coordinates; all zero without a shift"""
    img = np.zeros((H, H), dtype=np.int64)
    if shift:
        cnt = 0
        for hs in (slice(0, -WIN), slice(-WIN, -shift), slice(-shift, None)):
            for ws in (slice(0, -WIN), slice(-WIN, -shift), slice(-shift, None)):
                img[hs, ws] = cnt
                cnt += 1
    nw = H // WIN
    return img.reshape(nw, WIN, nw, WIN).transpose(0, 2, 1, 3).reshape(nw * nw, WIN * WIN)


def split_heads(win, C):
    """[B, windows, 64, 3C] -> q, k, v, each [B, windows, heads, 64, 24]: a qkv row is [3][heads][24]"""
    B, nwin = win.shape[:2]
    w = win.reshape(B, nwin, WIN * WIN, 3, C // HEAD_DIM, HEAD_DIM).transpose(3, 0, 1, 4, 2, 5)
    return w[0], w[1], w[2]


def join_heads(o):
    """[B, windows, heads, 64, 24] -> [B, windows, 64, C]"""
    B, nwin, heads = o.shape[:3]
    return o.transpose(0, 1, 3, 2, 4).reshape(B, nwin, WIN * WIN, heads * HEAD_DIM)


def window_attention(qkv, relb, B, H, C, shift):
    """qkv [B*H*H, 3C], relb [heads, 64, 64] -> softmax(q k^T / sqrt(24) + relb (+ -100 between regions)) v as
    [B*H*H, C], original token order, float64"""
    q, k, v = split_heads(partition(np.asarray(qkv, dtype=np.float64).reshape(B, H, H, 3 * C), H, shift), C)
    att = q @ k.swapaxes(-1, -2) * HEAD_DIM ** -0.5 + np.asarray(relb, dtype=np.float64)[None, None]
    if shift:
        reg = regions(H, shift)
        att = att + ((reg[:, None, :] != reg[:, :, None]) * -100.0)[None, :, None]
    att = np.exp(att - att.max(-1, keepdims=True))
    o = (att / att.sum(-1, keepdims=True)) @ v
    return merge(join_heads(o), H, shift).reshape(B * H * H, C)

"""Exact data for the attention kernels (csrc/vit.hip attention_kernel, csrc/htsat.hip swin_attention_kernel) and the case
table of tests/test_gpu_attention_exact.py.  numpy only: no GPU, no library.  tests/test_attention_exact_cases_cpu.py holds
every condition stated here, per case, and runs a float32 emulation of the kernel's loop over the same data.

The kernel (softmax_block and the loop around it): sc = dh^-0.5 * log2(e) in fp32; per 64-key block mnew = max(mrun, mx * sc),
alpha = exp2(mrun - mnew), p = exp2(fma(s, sc, -mnew)) with the bare instruction, l sums the fp32 p, the PV product sees
bf16(p), the output is bf16(oacc * (1.f / l)), round to nearest even.  Three families of inputs make that output known bit
for bit, whatever the accuracy of exp2 (2^0 = 1 and 2^-inf = 0 are all it has to get exactly right):

  selector   K[j] = 8 * a distinct +-1 code, Q[t] = K[pi(t)], V seeded normal bf16.  The target scores 64 dh, key j scores less
             by 128 * hamming(code j, code pi(t)); with every gap * sc >= 150 every other p is 0 in fp32 (flushed or not) and an
             earlier block is wiped by alpha = exp2(<= -150) = 0.  The target's p is 2^e, |e| <= half a unit in the last place
             of mnew (~3e-5): bf16(p) = 1, l = 1 + O(1e-4), and bf16(V (1 - O(1e-4))) = V, a rounding midpoint being 2^-9 away.
             Expected: o[b, t, h] = V[b, pi(t), h] as bits.  Pins the addressing: which key, which head, which channel, which
             k-slot of the PV product.
  uniform    Q = 0, K seeded normal, V integers in [-16, 16].  Every score is 0: p = 1 on every visible key, 0 on every masked
             one, l = n the visible count, the sum of V exact in fp32 in any order.  Expected: bf16(f32(sum) * (f32(1) / f32(n))),
             the kernel's own two operations.  Pins the masks: n = t + 1 (causal), clamp(lens[b], 1, T) on every row (lens).
  ties       selector codes, but a target code is shared by a group of 2 or 4 keys in different 64-key blocks where T allows; V
             integers in [-32, 32].  Every visible member gets bf16(p) = 1 (equal scores give equal p; alpha between their
             blocks is exp2(0) = 1): the output is the mean of the group's visible part.  Groups are cut on purpose by the
             causal mask and by lens.  The only family in which several blocks contribute through real QK^T scores.

HTSAT's window attention (head dim 24, one 64-key block, relative-position bias, cyclic shift by addressing, -100 between
shift regions) has its own three: `bias` (Q = K = 0, relb 0 at k = pi_h(q) and -1000 elsewhere), `code` (relb 0, K the key's
6-bit index, each bit four times as +-16: gap * 24^-0.5 * log2(e) >= 600) and `uniform` (the mean over the query's region:
exp2(-100 log2(e)) is 0 as bf16 and vanishes in the fp32 sum).  Its layout comes from tests/swin_window_ref.py."""
import collections
import functools
import math

import numpy as np

from tests import swin_window_ref as sw

KEY_BLOCK = 64
MIN_GAP = 150.0                                 # gap * sc at which exp2 is 0 in fp32, subnormals or not (2^-150 rounds to 0)
LOG2E = np.float32(1.4426950408889634)
FAMILIES = ("selector", "uniform", "ties")
SWIN_FAMILIES = ("bias", "code", "uniform")


def sc(dh):
    """softmax_block's scale: (dh == 64 ? 0.125f : 0.1118...f) * 1.4426950408889634f"""
    return np.float32(np.float32(0.125 if dh == 64 else 0.11180339887498948) * LOG2E)


def min_hamming(dh):
    """the code distance from which a non-target key's gap * sc is at least MIN_GAP (a differing channel costs 2 * 8 * 8)"""
    return math.ceil(MIN_GAP / (128.0 * float(sc(dh))))


def bf16_bits(x):
    """float32 -> bf16 bits, round to nearest even (finite values)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_f32(bits):
    return (np.asarray(bits).astype(np.uint32) << np.uint32(16)).view(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch of attention_bf16 / attention_cls (csrc/vit.hip), restated
# ---------------------------------------------------------------------------------------------------------------------
ENTRY_POINT = {"plain": "wise_attention_bf16", "dh": "wise_attention_dh_bf16", "causal": "wise_attention_causal_bf16",
               "lens": "wise_attention_lens_bf16", "cls": "wise_debug_attention_cls_bf16"}
ENTRY_MASK = {"plain": "none", "dh": "none", "causal": "causal", "lens": "lens", "cls": "cls"}


def instantiation(entry, T, dh=64):
    """attention_kernel<QT, CAUSAL, DH, PF, CLS> the entry point launches: head dim 80 -> QT 2; T <= 32 -> QT 2, else QT 4;
    the class-query form is QT 1"""
    if entry == "cls":
        return (1, False, 64, False, True)
    if dh == 80:
        return (2, False, 80, False, False)
    return (2 if T <= 32 else 4, entry == "causal", 64, False, False)


# instantiations in the source that no product path launches (the prefetch forms behind wise_debug_set_vit_streams)
DEBUG_ONLY_INSTANTIATIONS = ((3, False, 64, True, False), (2, False, 64, True, False))
# sizes an instantiation must be run at: its smallest, and the two sides of its last edge
EDGE_SIZES = {(2, False, 64, False, False): (1, 16, 17, 32), (4, False, 64, False, False): (33, 64, 65, 128, 129),
              (2, True, 64, False, False): (1, 16, 17, 32), (4, True, 64, False, False): (33, 64, 65, 128, 129),
              (2, False, 80, False, False): (1, 32, 33, 64, 65), (1, False, 64, False, True): (1, 2, 64, 65)}

Case = collections.namedtuple("Case", "entry family T dh sizes lens")        # sizes: ((B, H), ...); lens: per sequence, or None

T_QT2 = (1, 15, 16, 17, 31, 32)
T_QT4 = (33, 48, 49, 63, 64, 65, 127, 128, 129, 197, 257, 577)
T_CAUSAL = tuple(sorted(set(t for t in T_QT2 + T_QT4 if t <= 129) | {77}))
T_DH80 = (1, 31, 32, 33, 64, 65, 257)
T_LENS = (32, 64, 65, 200)
T_CLS = (1, 2, 50, 64, 65, 197)
SIZES = ((1, 1), (1, 3), (3, 1), (3, 3))


def lens_of(T):
    """one sequence per key count at an edge that fits, then 0 and T + 3, which the kernel clamps to 1 and T"""
    return tuple(sorted({v for v in (1, 15, 16, 17, 63, 64, 65, T - 1, T) if 1 <= v <= T})) + (0, T + 3)


def _cases():
    out = []
    for fam in FAMILIES:
        out += [Case("plain", fam, T, 64, SIZES, None) for T in T_QT2 + T_QT4]
        out += [Case("causal", fam, T, 64, SIZES, None) for T in T_CAUSAL]
        out += [Case("dh", fam, T, 80, SIZES, None) for T in T_DH80]
        out += [Case("lens", fam, T, 64, ((len(lens_of(T)), 1), (len(lens_of(T)), 3)), lens_of(T)) for T in T_LENS]
        out += [Case("cls", fam, T, 64, SIZES, None) for T in T_CLS]
    return tuple(out)


CASES = _cases()


def case_id(c):
    return f"{c.entry}-{c.family}-T{c.T}"


def case_seed(c):
    return 7919 * c.T + 101 * c.dh + 13 * FAMILIES.index(c.family) + len(c.entry)


# ---------------------------------------------------------------------------------------------------------------------
# plans: what is visible, the codes, who targets whom
# ---------------------------------------------------------------------------------------------------------------------
def visible(mask, T, lens_b=None):
    """[T]: the keys each query row sees — every mask here is a prefix, keys 0 .. n - 1"""
    if mask == "causal":
        return np.arange(1, T + 1)
    if mask == "lens":
        return np.full(T, min(max(int(lens_b), 1), T))
    return np.full(T, T)


def _rng(seed, *tag):
    return np.random.default_rng([seed, *tag])


def _codes(rng, n, dh):
    """n distinct +-1 codes of length dh at pairwise Hamming distance >= min_hamming(dh) (seeded draws until they are)"""
    while True:
        c = (rng.integers(0, 2, size=(n, dh)) * 2 - 1).astype(np.int32)
        if n == 1:
            return c
        g = c @ c.T
        np.fill_diagonal(g, -dh)
        if (dh - int(g.max())) // 2 >= min_hamming(dh):
            return c


def _cls_candidates(T):
    """targets of the class query, one per (batch, head) in turn: the first key, the last, the edges of every key block"""
    c = [0, T - 1]
    for blk in range(0, T, KEY_BLOCK):
        c += [blk, min(T, blk + KEY_BLOCK) - 1, min(T - 1, blk + 17)]
    return list(dict.fromkeys(c))


def _targets(rng, n, T, pair, cls):
    """pi [T], pi(t) < n[t]: seeded; per 32-query chunk one target in a key block before the query's own and one in a block
    after it (where visible), one query on key 0 and one on its last visible key"""
    pi = (rng.random(T) * n).astype(np.int64)
    if cls:
        cand = _cls_candidates(T)
        pi[0] = cand[pair % len(cand)]
        return pi
    taken = set()

    def force(t, k):
        pi[t] = k
        taken.add(t)

    for c0 in range(0, T, 32):
        qs = [int(t) for t in c0 + rng.permutation(min(T, c0 + 32) - c0)]
        t = next((t for t in qs if t not in taken and t >= KEY_BLOCK and n[t] > 0), None)
        if t is not None:
            force(t, int(rng.integers(0, min(n[t], t // KEY_BLOCK * KEY_BLOCK))))
        t = next((t for t in qs if t not in taken and n[t] > (t // KEY_BLOCK + 1) * KEY_BLOCK), None)
        if t is not None:
            force(t, int(rng.integers((t // KEY_BLOCK + 1) * KEY_BLOCK, n[t])))
    order = [int(t) for t in rng.permutation(T)]
    order.sort(key=lambda t: n[t] <= 1)                       # a query that sees one key has no choice: take it last
    t = next((t for t in order if t not in taken), None)
    if t is not None:
        force(t, 0)
    t = next((t for t in order if t not in taken), None)
    if t is not None:
        force(t, int(n[t]) - 1)
    return pi


@functools.lru_cache(maxsize=8)
def selector_plan(B, T, H, dh, mask, lens, seed):
    """{(b, h): (codes [T, dh], pi [T], n [T])}"""
    plan = {}
    for b in range(B):
        n = visible(mask, T, lens[b] if lens else None)
        for h in range(H):
            rng = _rng(seed, 1, b, h)
            plan[b, h] = (_codes(rng, T, dh), _targets(rng, n, T, b * H + h, mask == "cls"), n)
    return plan


def _pick(rng, s, lo, hi, used):
    """up to s unused keys of [lo, hi), from as many different key blocks as there are"""
    by_block = collections.defaultdict(list)
    for j in range(lo, hi):
        if j not in used:
            by_block[j // KEY_BLOCK].append(j)
    blocks = [int(x) for x in rng.permutation(sorted(by_block))]
    out, i = [], 0
    while len(out) < s and any(by_block[x] for x in blocks):
        free = by_block[blocks[i % len(blocks)]]
        if free:
            out.append(free.pop(int(rng.integers(0, len(free)))))
        i += 1
    used.update(out)
    return out


def _tie_pair(rng, n, T, dh, mask, pair):
    G = max(1, min(8, T // 4))
    nvis = int(n.max())
    used, groups, whole = set(), [], []
    for g in range(G):
        s = min(T, 4 if g % 2 else 2)
        if mask == "lens" and nvis < T and g % 2 == 0 and s >= 2:         # cut by lens on purpose: half visible, half not
            m = _pick(rng, (s + 1) // 2, 0, nvis, used)
            m += _pick(rng, s - len(m), nvis, T, used)
            whole.append(False)
        elif mask == "lens" and nvis - len([j for j in used if j < nvis]) >= s:
            m = _pick(rng, s, 0, nvis, used)                              # wholly visible
            whole.append(False)
        else:
            m = _pick(rng, s, 0, T, used)
            whole.append(True)
        if m:
            groups.append(sorted(m))
        else:
            whole.pop()
    G = len(groups)
    code_id = np.full(T, -1, dtype=np.int64)
    for g, m in enumerate(groups):
        code_id[m] = g
    rest = np.flatnonzero(code_id < 0)
    code_id[rest] = G + np.arange(rest.size)
    codes = _codes(rng, G + rest.size, dh)
    # targets: mostly groups with a visible member; on purpose every visible count of every group the mask can produce
    target = np.empty(T, dtype=np.int64)
    for t in range(T):
        gv = [g for g, m in enumerate(groups) if m[0] < n[t]]
        target[t] = gv[int(rng.integers(0, len(gv)))] if gv and rng.random() < 0.75 else code_id[int(rng.integers(0, n[t]))]
    if mask == "cls":
        target[0] = pair % G
        return codes, code_id, target, groups, whole
    taken = set()
    for g, m in enumerate(groups):
        for k in range(1, len(m) + 1):                        # queries that see exactly k members (n is non-decreasing in t)
            qs = [t for t in range(T) if t not in taken and sum(j < n[t] for j in m) == k]
            if qs:
                t = qs[int(rng.integers(0, len(qs)))]
                target[t] = g
                taken.add(t)
    return codes, code_id, target, groups, whole


@functools.lru_cache(maxsize=8)
def tie_plan(B, T, H, dh, mask, lens, seed):
    """{(b, h): (codes [ids, dh], code_id [T] of every key, target [T] code id of every query, groups, whole, n [T])};
    whole[g]: the group was drawn over all of 0 .. T - 1"""
    plan = {}
    for b in range(B):
        n = visible(mask, T, lens[b] if lens else None)
        for h in range(H):
            plan[b, h] = _tie_pair(_rng(seed, 2, b, h), n, T, dh, mask, b * H + h) + (n,)
    return plan


def tie_members(code_id, target_t, n_t):
    """the visible keys that carry query t's target code"""
    return np.flatnonzero((code_id == target_t) & (np.arange(code_id.size) < n_t))


# ---------------------------------------------------------------------------------------------------------------------
# builders: (B, T, H, dh, mask, lens, seed) -> qkv [B*T, 3*H*dh] bf16 bits, expected bf16 bits ([B*T, H*dh]; cls: [B, H*dh])
# ---------------------------------------------------------------------------------------------------------------------
def _pm(codes, mag_bits):
    """+-1 codes -> bf16 bits of +-magnitude"""
    return np.where(codes > 0, np.uint16(mag_bits), np.uint16(mag_bits | 0x8000)).astype(np.uint16)


PLUS8 = 0x4100
PLUS16 = 0x4180


def _normal_bits(rng, shape):
    return bf16_bits(rng.standard_normal(shape).astype(np.float32))


def _int_bits(v):
    return bf16_bits(v.astype(np.float32))                   # |v| <= 256: exact


def _assemble(q, k, v, exp, mask):
    """q, k, v, exp [B, T, H, dh] bits -> the packed rows"""
    B, T, H, dh = q.shape
    qkv = np.concatenate([x.reshape(B * T, H * dh) for x in (q, k, v)], axis=1)
    exp = exp[:, 0].reshape(B, H * dh) if mask == "cls" else exp.reshape(B * T, H * dh)
    return np.ascontiguousarray(qkv), np.ascontiguousarray(exp)


def build_selector(B, T, H, dh, mask, lens, seed):
    plan = selector_plan(B, T, H, dh, mask, lens, seed)
    q, k, v, e = (np.zeros((B, T, H, dh), dtype=np.uint16) for _ in range(4))
    for (b, h), (codes, pi, _) in plan.items():
        k[b, :, h] = _pm(codes, PLUS8)
        q[b, :, h] = k[b, pi, h]
        v[b, :, h] = _normal_bits(_rng(seed, 3, b, h), (T, dh))
        e[b, :, h] = v[b, pi, h]
    return _assemble(q, k, v, e, mask)


def uniform_values(B, T, H, dh, seed):
    """V of the uniform family as integers [B, T, H, dh]"""
    return _rng(seed, 4).integers(-16, 17, size=(B, T, H, dh))


def build_uniform(B, T, H, dh, mask, lens, seed):
    vi = uniform_values(B, T, H, dh, seed)
    q = np.zeros((B, T, H, dh), dtype=np.uint16)
    k = _normal_bits(_rng(seed, 5), (B, T, H, dh))
    e = np.zeros_like(q)
    for b in range(B):
        n = visible(mask, T, lens[b] if lens else None)
        total = np.cumsum(vi[b], axis=0)[n - 1]                                        # [T, H, dh]: the sum over keys < n[t]
        e[b] = bf16_bits(total.astype(np.float32) * (np.float32(1) / n.astype(np.float32))[:, None, None])
    return _assemble(q, k, _int_bits(vi), e, mask)


def tie_values(B, T, H, dh, seed):
    return _rng(seed, 6).integers(-32, 33, size=(B, T, H, dh))


def build_ties(B, T, H, dh, mask, lens, seed):
    plan = tie_plan(B, T, H, dh, mask, lens, seed)
    vi = tie_values(B, T, H, dh, seed)
    q, k, e = (np.zeros((B, T, H, dh), dtype=np.uint16) for _ in range(3))
    for (b, h), (codes, code_id, target, _, _, n) in plan.items():
        k[b, :, h] = _pm(codes[code_id], PLUS8)
        q[b, :, h] = _pm(codes[target], PLUS8)
        for t in range(1 if mask == "cls" else T):
            m = tie_members(code_id, target[t], n[t])
            e[b, t, h] = bf16_bits((vi[b, m, h].sum(axis=0) / m.size).astype(np.float32))
    return _assemble(q, k, _int_bits(vi), e, mask)


BUILDERS = {"selector": build_selector, "uniform": build_uniform, "ties": build_ties}


def build_case(c, B, H):
    """qkv, expected of case c at (B, H)"""
    return BUILDERS[c.family](B, c.T, H, c.dh, ENTRY_MASK[c.entry], c.lens, case_seed(c))


# ---------------------------------------------------------------------------------------------------------------------
# HTSAT window attention: (family, B, H, C, shift, seed) -> qkv [B*H*H, 3C] bits, relb [C/24, 64, 64] fp32, expected [B*H*H, C] bits
# ---------------------------------------------------------------------------------------------------------------------
SwinCase = collections.namedtuple("SwinCase", "family C H shift")
SWIN_CASES = tuple(SwinCase(f, C, H, s) for f in SWIN_FAMILIES for C in (96, 192, 384) for H in (8, 16) for s in (0, 4))
SWIN_BATCHES = (1, 3)
SWIN_BIAS_OFF = -1000.0


def swin_case_id(c):
    return f"swin-{c.family}-C{c.C}-H{c.H}-shift{c.shift}"


def swin_case_seed(c):
    return 31 * c.C + 7 * c.H + c.shift + 1000 * SWIN_FAMILIES.index(c.family)


def quadrant(p):
    """the 4 x 4 quarter of an 8 x 8 window token p lies in: tokens of one quarter share a shift region in every window"""
    return ((np.asarray(p) >> 3) >= 4) * 2 + ((np.asarray(p) & 7) >= 4)


def swin_bias_targets(heads, shift, seed):
    """pi [heads, 64]: per head (relb is shared by every image and window); inside the query's quarter when shifted"""
    rng = _rng(seed, 7)
    pi = rng.integers(0, 64, size=(heads, 64))
    if shift:
        tok = np.arange(64)
        for h in range(heads):
            for qd in range(4):
                idx = tok[quadrant(tok) == qd]
                pi[h, idx] = rng.choice(idx, size=idx.size)
    return pi


def swin_code_targets(B, H, C, shift, seed):
    """pi [B, windows, heads, 64]: inside the query's own region of its own window"""
    rng = _rng(seed, 8)
    reg = sw.regions(H, shift)
    heads = C // sw.HEAD_DIM
    pi = np.zeros((B, reg.shape[0], heads, 64), dtype=np.int64)
    for w in range(reg.shape[0]):
        for r in np.unique(reg[w]):
            idx = np.flatnonzero(reg[w] == r)
            pi[:, w, :, idx] = rng.choice(idx, size=(idx.size, B, heads))
    return pi


def swin_key_codes():
    """[64, 24] +-1: bit i of the key's index, four times"""
    j = np.arange(64)
    return np.repeat(((j[:, None] >> np.arange(6)[None]) & 1) * 2 - 1, 4, axis=1)


def build_swin(family, B, H, C, shift, seed):
    heads, nwin = C // sw.HEAD_DIM, (H // 8) ** 2
    shape = (B, nwin, heads, 64, sw.HEAD_DIM)
    rng = _rng(seed, 9)
    relb = np.zeros((heads, 64, 64), dtype=np.float32)
    q = np.zeros(shape, dtype=np.uint16)
    if family == "bias":
        pi = swin_bias_targets(heads, shift, seed)
        relb[:] = SWIN_BIAS_OFF
        relb[np.arange(heads)[:, None], np.arange(64)[None], pi] = 0.0
        k = np.zeros(shape, dtype=np.uint16)
        v = _normal_bits(rng, shape)
        e = np.stack([v[:, :, h, pi[h]] for h in range(heads)], axis=2)
    elif family == "code":
        pi = swin_code_targets(B, H, C, shift, seed)
        k = np.broadcast_to(_pm(swin_key_codes(), PLUS16), shape).copy()
        q = np.take_along_axis(k, pi[..., None], axis=3)
        v = _normal_bits(rng, shape)
        e = np.take_along_axis(v, pi[..., None], axis=3)
    else:
        assert family == "uniform"
        k = _normal_bits(rng, shape)
        vi = rng.integers(-16, 17, size=shape)
        v = _int_bits(vi)
        reg = sw.regions(H, shift)
        same = (reg[:, :, None] == reg[:, None, :]).astype(np.int64)                   # [windows, 64 q, 64 k]
        total = np.einsum("wqk,bwhkd->bwhqd", same, vi)
        n = same.sum(-1).astype(np.float32)                                            # [windows, 64]
        e = bf16_bits(total.astype(np.float32) * (np.float32(1) / n)[None, :, None, :, None])
    rows = np.concatenate([sw.join_heads(x) for x in (q, k, v)], axis=-1)              # [B, windows, 64, 3C]
    qkv = sw.merge(rows, H, shift).reshape(B * H * H, 3 * C)
    exp = sw.merge(sw.join_heads(e), H, shift).reshape(B * H * H, C)
    return np.ascontiguousarray(qkv), relb, np.ascontiguousarray(exp)


def region_sizes(H, shift):
    """the sizes of the regions that occur in the windows of an H x H grid"""
    reg = sw.regions(H, shift)
    return sorted({int((reg[w] == r).sum()) for w in range(reg.shape[0]) for r in np.unique(reg[w])})

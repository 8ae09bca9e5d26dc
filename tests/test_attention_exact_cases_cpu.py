"""What the expectations of tests/attention_exact_cases.py rest on, for every case of its table, without a GPU: distinct codes
whose gaps drive exp2 to 0, targets that respect the mask and reach the first, the last and the neighbouring key blocks, tie
groups across blocks with exact sums — and a numpy float32 emulation of the kernel's loop AS WRITTEN (64-key blocks, running
maximum, alpha, fp32 l, bf16 p; csrc/vit.hip softmax_block and the loop around it) that must give the expected bits with
exp2 exact and with exp2 off by two units in the last place either way.  2^0 = 1 and 2^-inf = 0 stay exact in the perturbed
runs: the uniform family rests on those two values and on nothing else of the instruction."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import attention_exact_cases as ac
from tests import swin_window_ref as sw

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "wise_amd" / "csrc"
_IDS = [ac.case_id(c) for c in ac.CASES]
_SWIN_IDS = [ac.swin_case_id(c) for c in ac.SWIN_CASES]


# ---------------------------------------------------------------------------------------------------------------------
# the table against the source
# ---------------------------------------------------------------------------------------------------------------------
def _launched_instantiations():
    """every attention_kernel<...> csrc/vit.hip launches, as (QT, CAUSAL, DH, PF, CLS) with the template's defaults"""
    text = (CSRC / "vit.hip").read_text()
    out = set()
    for args in re.findall(r"hipLaunchKernelGGL\(\(attention_kernel<([^>]*)>\)", text):
        a = [x.strip() for x in args.split(",")]
        a += ["64", "false", "false"][len(a) - 2:]
        out.add((int(a[0]), a[1] == "true", int(a[2]), a[3] == "true", a[4] == "true"))
    return out


def test_every_instantiation_the_product_launches_is_in_the_table_at_its_edges():
    launched = _launched_instantiations()
    assert len(launched) == 8, launched                     # the parser sees them all (8 when this was written)
    ran = {}
    for c in ac.CASES:
        ran.setdefault((ac.instantiation(c.entry, c.T, c.dh), c.family), set()).add(c.T)
    for inst in sorted(launched - set(ac.DEBUG_ONLY_INSTANTIATIONS)):
        assert inst in ac.EDGE_SIZES, f"attention_kernel<{inst}> has no case in tests/attention_exact_cases.py"
        for fam in ac.FAMILIES:
            assert set(ac.EDGE_SIZES[inst]) <= ran.get((inst, fam), set()), (inst, fam)
    assert set(ac.EDGE_SIZES) <= launched and set(ac.DEBUG_ONLY_INSTANTIATIONS) <= launched
    # the dispatch as restated is the dispatch as written
    text = (CSRC / "vit.hip").read_text()
    assert "(T <= 32 ? 2 : 4)" in text and "attention_kernel<2, false, 80>" in text and "attention_kernel<1, false, 64, false, true>" in text
    # and the window kernel has one launch form, which the debug entry point repeats
    htsat = (CSRC / "htsat.hip").read_text()
    launches = re.findall(r"hipLaunchKernelGGL\(swin_attention_kernel, dim3\(\(unsigned\)\(\(items \+ 3\) / 4\)\), dim3\(256\), 0, st,\s*qkv, B, H,\s*H, C, heads, shift, (\w+), (\w+)\)", htsat)
    assert len(launches) == 3 and "wise_debug_swin_attention" in htsat, launches


def test_the_ledger_notices_an_instantiation_that_leaves_the_table():
    ran = {ac.instantiation(c.entry, c.T, c.dh) for c in ac.CASES if c.entry != "dh"}
    assert _launched_instantiations() - set(ac.DEBUG_ONLY_INSTANTIATIONS) - ran == {(2, False, 80, False, False)}


def test_case_table_is_what_the_sizes_say():
    by = {}
    for c in ac.CASES:
        by.setdefault((c.entry, c.family), []).append(c.T)
    for fam in ac.FAMILIES:
        assert by["plain", fam] == [1, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64, 65, 127, 128, 129, 197, 257, 577]
        assert by["causal", fam] == [1, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64, 65, 77, 127, 128, 129]
        assert by["dh", fam] == [1, 31, 32, 33, 64, 65, 257]
        assert by["lens", fam] == [32, 64, 65, 200]
        assert by["cls", fam] == [1, 2, 50, 64, 65, 197]
    assert ac.lens_of(32) == (1, 15, 16, 17, 31, 32, 0, 35)
    assert ac.lens_of(200) == (1, 15, 16, 17, 63, 64, 65, 199, 200, 0, 203)
    assert {(c.C, c.H, c.shift) for c in ac.SWIN_CASES} == {(C, H, s) for C in (96, 192, 384) for H in (8, 16) for s in (0, 4)}
    assert len(ac.SWIN_CASES) == 36 and ac.SWIN_BATCHES == (1, 3)
    for T in (1, 32):
        assert ac.instantiation("plain", T)[0] == 2 and ac.instantiation("causal", T)[:2] == (2, True)
    assert ac.instantiation("plain", 33)[0] == 4 and ac.instantiation("dh", 257, 80)[0] == 2


def test_bf16_helpers_round_to_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-5, 257.0, 4.015625], dtype=np.float32)
    assert list(ac.bf16_f32(ac.bf16_bits(x))) == [1.0, 1.0, 1.015625, -1.0, np.float32(3.0040741e-05), 256.0, 4.0]
    assert ac.bf16_bits(np.float32(8))[()] == ac.PLUS8 and ac.bf16_bits(np.float32(-16))[()] == ac.PLUS16 | 0x8000


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's loop in numpy float32
# ---------------------------------------------------------------------------------------------------------------------
def _exp2(x, ulps):
    """2^x in fp32, `ulps` units in the last place off — but exact at x = 0 and x = -inf, and a result that underflows to 0
    (x <= -150) stays 0: with alpha one subnormal step above 0 the wiped blocks would leave a signed dust that decides the
    sign of an output of exactly 0"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(under="ignore"):
        y = np.exp2(x.astype(np.float64)).astype(np.float32)
    exact = (x == 0) | np.isneginf(x) | (y == 0)
    z = y
    for _ in range(abs(ulps)):
        z = np.nextafter(z, np.float32(np.inf if ulps > 0 else 0.0))
    return np.where(exact, y, z).astype(np.float32)


def emulate(q, k, v, n, dh, ulps=0):
    """one (batch, head): q, k, v [T, dh] fp32 (bf16 values), n [T] visible keys per query -> bf16 bits [T, dh].  Key blocks
    a query sees nothing of are not run for it (the causal form stops at the chunk's own block)."""
    T = q.shape[0]
    scale = ac.sc(dh)
    mrun = np.full(T, -np.inf, dtype=np.float32)
    lrun = np.zeros(T, dtype=np.float32)
    oacc = np.zeros((T, dh), dtype=np.float32)
    for kb in range((int(n.max()) + 63) // 64):
        keys = np.arange(kb * 64, min(kb * 64 + 64, k.shape[0]))
        live = n > kb * 64
        s = (q @ k[keys].T).astype(np.float32)                                       # integers below 2^13: exact
        s = np.where(keys[None, :] >= n[:, None], np.float32(-np.inf), s)
        mx = s.max(axis=1)
        with np.errstate(all="ignore"):
            mnew = np.maximum(mrun, (mx * scale).astype(np.float32))
            alpha = _exp2(np.where(np.isneginf(mrun), np.float32(-np.inf), mrun - mnew), ulps)
            arg = (s.astype(np.float64) * np.float64(scale) - mnew[:, None].astype(np.float64)).astype(np.float32)   # one rounding: the fma
        p = np.where(live[:, None], _exp2(arg, ulps), np.float32(0))                # (rows that do not run this block: dropped below)
        pb = ac.bf16_f32(ac.bf16_bits(p))
        l_new = (lrun * alpha + p.sum(axis=1, dtype=np.float32)).astype(np.float32)
        o_new = (oacc * alpha[:, None] + (pb @ v[keys]).astype(np.float32)).astype(np.float32)
        mrun = np.where(live, mnew, mrun)
        lrun = np.where(live, l_new, lrun)
        oacc = np.where(live[:, None], o_new, oacc)
    inv = (np.float32(1) / lrun).astype(np.float32)
    return ac.bf16_bits(oacc * inv[:, None])


def _split(qkv, B, T, H, dh):
    x = ac.bf16_f32(qkv).reshape(B, T, 3, H, dh)
    return x[:, :, 0], x[:, :, 1], x[:, :, 2]


@pytest.mark.parametrize("c", ac.CASES, ids=_IDS)
def test_emulated_loop_gives_the_expected_bits(c):
    """exp2 exact, two units high, two units low: the same bits, the expected ones (largest (B, H) of the case)"""
    B, H = c.sizes[-1]
    mask = ac.ENTRY_MASK[c.entry]
    qkv, exp = ac.build_case(c, B, H)
    assert qkv.shape == (B * c.T, 3 * H * c.dh) and qkv.dtype == np.uint16 and exp.dtype == np.uint16
    q, k, v = _split(qkv, B, c.T, H, c.dh)
    exp = exp.reshape(B, 1 if mask == "cls" else c.T, H, c.dh)
    for b in range(B):
        n = ac.visible(mask, c.T, c.lens[b] if c.lens else None)
        for h in range(H):
            for ulps in (0, 2, -2):
                got = emulate(q[b, :, h], k[b, :, h], v[b, :, h], n, c.dh, ulps)
                got = got[:1] if mask == "cls" else got
                assert np.array_equal(got, exp[b, :, h]), (ac.case_id(c), b, h, ulps, np.argwhere(got != exp[b, :, h])[:3])


def test_emulation_notices_what_the_suite_is_for():
    """the faults the families are there for change the emulated bits: a mask off by one, a key counted twice"""
    c = next(x for x in ac.CASES if x.entry == "causal" and x.family == "uniform" and x.T == 65)
    qkv, exp = ac.build_case(c, 1, 1)
    q, k, v = _split(qkv, 1, 65, 1, 64)
    n = ac.visible("causal", 65)
    assert np.array_equal(emulate(q[0, :, 0], k[0, :, 0], v[0, :, 0], n, 64), exp.reshape(65, 64))
    off = emulate(q[0, :, 0], k[0, :, 0], v[0, :, 0], np.minimum(n + 1, 65), 64)
    assert (off != exp.reshape(65, 64)).any(axis=1).sum() >= 60
    c = next(x for x in ac.CASES if x.entry == "plain" and x.family == "ties" and x.T == 65)
    qkv, exp = ac.build_case(c, 1, 1)
    q, k, v = _split(qkv, 1, 65, 1, 64)
    twice = emulate(q[0, :, 0], np.concatenate([k[0, :, 0], k[0, -1:, 0]]), np.concatenate([v[0, :, 0], v[0, -1:, 0]]), np.full(65, 66), 64)
    assert (twice != exp.reshape(65, 64)).any()


# ---------------------------------------------------------------------------------------------------------------------
# the conditions, case by case
# ---------------------------------------------------------------------------------------------------------------------
def _min_gap(codes, dh):
    g = codes @ codes.T
    np.fill_diagonal(g, -dh)
    return 64.0 * (dh - int(g.max())) * float(ac.sc(dh))              # 8 * 8 * (dh - dot): the score gap, scaled


def _blocks(keys):
    return {int(j) // 64 for j in keys}


@pytest.mark.parametrize("c", [c for c in ac.CASES if c.family == "selector"], ids=[i for i, c in zip(_IDS, ac.CASES) if c.family == "selector"])
def test_selector_conditions(c):
    mask = ac.ENTRY_MASK[c.entry]
    first = last = 0
    for B, H in c.sizes:
        plan = ac.selector_plan(B, c.T, H, c.dh, mask, c.lens, ac.case_seed(c))
        pis = []
        for (b, h), (codes, pi, n) in plan.items():
            assert codes.shape == (c.T, c.dh) and set(np.unique(codes)) <= {-1, 1}
            if c.T > 1:
                assert _min_gap(codes, c.dh) >= ac.MIN_GAP, (b, h)                  # distinct, and far enough apart
            assert np.array_equal(n, ac.visible(mask, c.T, c.lens[b] if c.lens else None))
            assert (pi >= 0).all() and (pi < n).all()                               # the mask is respected
            rows = np.arange(1) if mask == "cls" else np.arange(c.T)
            first += int((pi[rows] == 0).sum())
            last += int((pi[rows] == n[rows] - 1).sum())
            if n.max() > 2:                                                         # (a sequence of one key leaves no choice)
                pis.append(tuple(pi))
            if mask != "cls":
                assert (pi == 0).any() and (pi == n - 1).any()
                if c.T > 1 and mask != "causal":
                    assert ((pi == n - 1) & (n > 1)).any() or n.max() == 1
                for c0 in range(0, c.T, 32):                                        # both sides across blocks, per query chunk
                    ts = np.arange(c0, min(c.T, c0 + 32))
                    own = ts // 64
                    if ts.size >= 4 and (own > 0).any():
                        assert (pi[ts] // 64 < own).any(), (b, h, c0)
                    if ts.size >= 4 and (n[ts] > (own + 1) * 64).any():
                        assert (pi[ts] // 64 > own).any(), (b, h, c0)
        if B * H > 1 and c.T > 2:
            assert len(set(pis)) == len(pis)                                        # differs per (batch, head)
    assert first and last
    if mask == "cls" and c.T > 64:
        B, H = c.sizes[-1]
        plan = ac.selector_plan(B, c.T, H, c.dh, mask, c.lens, ac.case_seed(c))
        assert len({int(pi[0]) // 64 for _, pi, _ in plan.values()}) == (c.T + 63) // 64


@pytest.mark.parametrize("c", [c for c in ac.CASES if c.family == "ties"], ids=[i for i, c in zip(_IDS, ac.CASES) if c.family == "ties"])
def test_tie_conditions(c):
    mask = ac.ENTRY_MASK[c.entry]
    counts_seen = set()
    for B, H in c.sizes:
        plan = ac.tie_plan(B, c.T, H, c.dh, mask, c.lens, ac.case_seed(c))
        vi = ac.tie_values(B, c.T, H, c.dh, ac.case_seed(c))
        assert np.abs(vi).max() <= 32
        _, exp = ac.build_case(c, B, H)
        exp = ac.bf16_f32(exp).reshape(B, 1 if mask == "cls" else c.T, H, c.dh)
        for (b, h), (codes, code_id, target, groups, whole, n) in plan.items():
            if codes.shape[0] > 1:
                assert _min_gap(codes, c.dh) >= ac.MIN_GAP
            assert sorted(j for m in groups for j in m) == sorted(set(j for m in groups for j in m))      # groups are disjoint
            for g, m in enumerate(groups):
                assert (code_id[m] == g).all() and int((code_id == g).sum()) == len(m)
                if c.T > 64 and whole[g]:
                    # spans blocks: as many as it has members, or every full block (a tail block of a few keys may be used up)
                    assert len(_blocks(m)) >= min(len(m), max(c.T // 64, 2 if g == 0 else 1)), (b, h, m)
            if c.T >= 4:
                assert any(len(m) >= 2 for m in groups)
            if int(n.max()) >= 80:                                                  # (a second block of a few keys may be used up)
                assert any(len(_blocks([j for j in m if j < n.max()])) >= 2 for m in groups), (b, h)
            if mask == "lens" and 1 < int(n.max()) < c.T:
                assert any(0 < sum(j < n.max() for j in m) < len(m) for m in groups), (b, h)                # cut by lens
            for t in range(1 if mask == "cls" else c.T):
                m = ac.tie_members(code_id, target[t], n[t])
                assert m.size >= 1
                counts_seen.add((int(m.size), int((code_id == target[t]).sum())))
                mean = vi[b, m, h].astype(np.float64).sum(axis=0) / m.size                                  # exact sum, float64 mean
                assert np.array_equal(vi[b, m, h].sum(axis=0), vi[b, m, h].astype(np.float32).sum(axis=0, dtype=np.float32))
                # the expectation is the nearest bf16 of the mean, and no mean is within 2^-12 (relative) of a rounding midpoint:
                # the factor 1 + O(1e-4) that 1 / l leaves cannot move it
                got = exp[b, t, h].astype(np.float64)
                with np.errstate(divide="ignore"):
                    half = np.where(got == 0, 0.0, 2.0 ** (np.floor(np.log2(np.abs(got))) - 8))             # half a bf16 step at got
                assert (np.abs(got - mean) <= half).all()
                assert (half - np.abs(got - mean) >= np.abs(mean) * 2.0 ** -12)[got != mean].all()
    if mask == "causal" and c.T >= 64:
        assert {(1, 2), (2, 2), (1, 4), (2, 4), (3, 4), (4, 4)} <= counts_seen, counts_seen                 # every cut of every size
    if mask == "none" and c.T >= 16:
        assert {(2, 2), (4, 4)} <= counts_seen


@pytest.mark.parametrize("c", [c for c in ac.CASES if c.family == "uniform"], ids=[i for i, c in zip(_IDS, ac.CASES) if c.family == "uniform"])
def test_uniform_conditions(c):
    mask = ac.ENTRY_MASK[c.entry]
    B, H = c.sizes[-1]
    qkv, exp = ac.build_case(c, B, H)
    q, k, v = _split(qkv, B, c.T, H, c.dh)
    assert not q.any() and np.abs(v).max() <= 16 and np.array_equal(v, np.round(v))
    assert np.unique(k).size > min(100, k.size // 4)                                    # K is arbitrary, and is not looked at
    exp = ac.bf16_f32(exp).reshape(B, 1 if mask == "cls" else c.T, H, c.dh)
    for b in range(B):
        n = ac.visible(mask, c.T, c.lens[b] if c.lens else None)
        if mask == "causal":
            assert np.array_equal(n, np.arange(c.T) + 1)
        if mask == "lens":
            assert (n == min(max(c.lens[b], 1), c.T)).all()
        for t in range(exp.shape[1]):
            total = v[b, :n[t]].astype(np.float64).sum(axis=0)                          # [H, dh]
            assert np.array_equal(total, v[b, :n[t]][::-1].sum(axis=0, dtype=np.float32))        # exact in fp32, in another order
            assert (np.abs(exp[b, t] - total / n[t]) <= np.abs(total / n[t]) * 2.0 ** -8).all()    # one bf16 step of the mean at most
            if n[t] & (n[t] - 1) == 0:
                want = ac.bf16_f32(ac.bf16_bits((total / n[t]).astype(np.float32)))
                assert np.array_equal(exp[b, t], want)                                  # power of two: the quotient is exact


# ---------------------------------------------------------------------------------------------------------------------
# HTSAT window attention
# ---------------------------------------------------------------------------------------------------------------------
def test_region_sizes_that_occur():
    """8 x 8 grid, shift 4: the one window is the grid's last row AND column of windows — four regions of 16 (slice(0, -8) is
    empty: regions 4, 5, 7, 8).  16 x 16: one window whole, two cut in halves, one in quarters.  (The nine regions of the
    general case need H >= 16.)"""
    assert ac.region_sizes(8, 0) == [64] and ac.region_sizes(16, 0) == [64]
    assert ac.region_sizes(8, 4) == [16] and sorted(np.unique(sw.regions(8, 4))) == [4, 5, 7, 8]
    assert ac.region_sizes(16, 4) == [16, 32, 64] and len(np.unique(sw.regions(16, 4))) == 9
    reg = sw.regions(16, 4)
    assert [len(np.unique(reg[w])) for w in range(4)] == [1, 2, 2, 4]
    # the kernel's region_of (csrc/htsat.hip), token by token
    for H in (8, 16):
        reg = sw.regions(H, 4)
        nw = H // 8
        for w in range(nw * nw):
            for p in range(64):
                ys, xs = (w // nw) * 8 + (p >> 3), (w % nw) * 8 + (p & 7)
                assert reg[w, p] == ((ys >= H - 8) + (ys >= H - 4)) * 3 + (xs >= H - 8) + (xs >= H - 4)


def test_partition_and_merge_are_inverse_and_follow_row_of():
    for H, shift in ((8, 0), (8, 4), (16, 0), (16, 4)):
        x = np.arange(2 * H * H * 3).reshape(2, H, H, 3)
        w = sw.partition(x, H, shift)
        assert np.array_equal(sw.merge(w, H, shift), x)
        nw = H // 8
        for win in range(nw * nw):
            for p in (0, 7, 27, 36, 63):                       # the kernel's row_of
                y, xx = ((win // nw) * 8 + (p >> 3) + shift) % H, ((win % nw) * 8 + (p & 7) + shift) % H
                assert np.array_equal(w[1, win, p], x[1, y, xx])


def _swin_emulate(qkv, relb, B, H, C, shift, ulps):
    """swin_attention_kernel in float32: s = (q k^T) * 24^-0.5 + relb (- 100 across regions), times log2(e); p = exp2(s - max);
    bf16(p) into the PV product; bf16(o * (1.f / sum p))"""
    q, k, v = sw.split_heads(sw.partition(ac.bf16_f32(qkv).reshape(B, H, H, 3 * C), H, shift), C)
    s = (q @ k.swapaxes(-1, -2)).astype(np.float32) * np.float32(0.20412414523193154) + relb[None, None]
    if shift:
        reg = sw.regions(H, shift)
        s = s + np.where(reg[:, :, None] != reg[:, None, :], np.float32(-100), np.float32(0))[None, :, None]
    s = (s.astype(np.float32) * ac.LOG2E).astype(np.float32)
    p = _exp2(s - s.max(-1, keepdims=True), ulps)
    pb = ac.bf16_f32(ac.bf16_bits(p))
    o = (pb @ v).astype(np.float32) * (np.float32(1) / p.sum(-1, dtype=np.float32))[..., None]
    return sw.merge(sw.join_heads(ac.bf16_bits(o)), H, shift).reshape(B * H * H, C)


@pytest.mark.parametrize("c", ac.SWIN_CASES, ids=_SWIN_IDS)
def test_swin_conditions_and_emulation(c):
    B = ac.SWIN_BATCHES[-1]
    seed = ac.swin_case_seed(c)
    heads = c.C // 24
    qkv, relb, exp = ac.build_swin(c.family, B, c.H, c.C, c.shift, seed)
    assert qkv.shape == (B * c.H * c.H, 3 * c.C) and relb.shape == (heads, 64, 64) and exp.shape == (B * c.H * c.H, c.C)
    reg = sw.regions(c.H, c.shift)
    if c.family == "bias":
        pi = ac.swin_bias_targets(heads, c.shift, seed)
        assert (reg[:, pi] == reg[:, np.arange(64)][:, None, :]).all()                  # the target stays in the query's region
        assert len({tuple(r) for r in pi}) == heads and not (pi == np.arange(64)).all(axis=1).any()
        assert (np.sort(relb, axis=-1)[..., -1] == 0).all() and (np.sort(relb, axis=-1)[..., -2] == ac.SWIN_BIAS_OFF).all()
        assert {int(x) // 16 for x in pi.ravel()} == {0, 1, 2, 3}                       # all four key tiles
    elif c.family == "code":
        pi = ac.swin_code_targets(B, c.H, c.C, c.shift, seed)
        assert (np.take_along_axis(np.broadcast_to(reg[None, :, None, :], pi.shape), pi, axis=-1) == reg[None, :, None, :]).all()
        codes = ac.swin_key_codes()
        g = codes @ codes.T
        np.fill_diagonal(g, -24)
        assert codes.shape == (64, 24) and 256.0 * (24 - g.max()) * 24 ** -0.5 * float(ac.LOG2E) >= 600.0
        assert not relb.any()
    else:
        assert not relb.any() and ac.region_sizes(c.H, c.shift) == {(8, 0): [64], (16, 0): [64], (8, 4): [16], (16, 4): [16, 32, 64]}[c.H, c.shift]
        # exp2(-100 log2 e) is 0 as bf16 and vanishes beside a sum of at least 1
        tiny = np.exp2(np.float64(np.float32(-100) * ac.LOG2E))
        assert ac.bf16_bits(np.float32(tiny))[()] == 0 and np.float32(1) + np.float32(64 * tiny) == np.float32(1)
    for ulps in (0, 2, -2):
        got = _swin_emulate(qkv, relb, B, c.H, c.C, c.shift, ulps)
        assert np.array_equal(got, exp), (ac.swin_case_id(c), ulps, np.argwhere(got != exp)[:3])
    # and the float64 statement of the layout the tolerance test uses agrees to within one bf16 step
    ref = sw.window_attention(ac.bf16_f32(qkv), relb, B, c.H, c.C, c.shift)
    e = ac.bf16_f32(exp).astype(np.float64)
    assert (np.abs(e - ref) <= np.abs(ref) * 2.0 ** -8 + 1e-30).all()

"""-m gpu: every attention form the towers launch, on data whose output is known bit for bit (tests/attention_exact_cases.py).

attention_kernel of csrc/vit.hip through wise_attention_bf16 / _dh_bf16 / _causal_bf16 / _lens_bf16 and the class-query form
through the debug library (wise_debug_attention_cls_bf16); swin_attention_kernel of csrc/htsat.hip through
wise_debug_swin_attention, which launches it as the tower does.  Three families per form — selector (one softmax weight is 1,
the rest 0: the addressing), uniform (every visible weight equal: the masks and the count), ties (a group of equal scores
across key blocks: the running maximum and alpha) — and for the window kernel bias / code / uniform.  Why each expectation
holds whatever exp2's accuracy is derived in the case module and held, case by case, by tests/test_attention_exact_cases_cpu.py,
which also runs a float32 emulation of the loop on the same data.

Every output sits between 128 guard rows of the NaN pattern 0x7FC1 in front and behind, which must come back untouched, and
is itself pre-filled with the pattern: an element nobody writes fails.  Comparison is torch.equal on the int16 views.
wise_attention_lens_bf16 clamps lens[b] to 1 .. T; lens = 0 and lens = T + 3 are in the table to pin that.

Seen on an MI355X: every family is bit-exact, the uniform one included at visible counts that are no power of two — 1.f / l is
the correctly rounded quotient, so nothing is held to a bf16 step instead of equality.  What value tests cannot see: the zeroing
of V rows past the last key (a masked key's weight is exactly 0 and the clamped row it would read is finite), and which of the
two coordinates of a shift region is called ry and which rx (the id is a label; the partition is the same)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import attention_exact_cases as ac
from tests.gemm_tile_check import where as _where
from wise_amd import _lib

pytestmark = pytest.mark.gpu

_P = C.c_void_p
GUARD_ROWS = 128
BF16_GUARD = 0x7FC1             # a NaN no kernel produces


@functools.lru_cache(maxsize=None)
def _dbg():
    d = _lib.load_debug()
    d.wise_debug_attention_cls_bf16.argtypes = [_P, C.c_int, C.c_int, C.c_int, _P, _P]
    d.wise_debug_attention_cls_bf16.restype = C.c_int
    d.wise_debug_swin_attention.argtypes = [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]
    d.wise_debug_swin_attention.restype = C.c_int
    return d


class _Guarded:
    """[rows, N] bf16 between GUARD_ROWS guard rows in front and behind, all of it filled with the NaN pattern"""

    def __init__(self, rows, N):
        self.bits = torch.full((rows + 2 * GUARD_ROWS, N), BF16_GUARD, dtype=torch.int16, device="cuda")
        self.body = self.bits[GUARD_ROWS:GUARD_ROWS + rows]

    def intact(self):
        g = GUARD_ROWS
        return bool((self.bits[:g] == BF16_GUARD).all()) and bool((self.bits[-g:] == BF16_GUARD).all())


def _dev(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda()


def _assert_bits(out, exp, what, rows_per_b, dh):
    """out.body against the expected bits; on failure the first (b, t, h, channel)"""
    assert out.intact(), f"{what}: guard rows written"
    want = _dev(exp)
    if not torch.equal(out.body, want):
        bad = out.body != want
        r, c = (int(x) for x in bad.nonzero()[0])
        unwritten = int((out.body == BF16_GUARD).sum())
        raise AssertionError(f"{_where(bad, what)}: b={r // rows_per_b} t={r % rows_per_b} h={c // dh} channel={c % dh}, "
                             f"got 0x{int(out.body[r, c]) & 0xFFFF:04X} want 0x{int(want[r, c]) & 0xFFFF:04X}; {unwritten} elements never written")


def _launch(c, B, H, qkv, o):
    T, st = c.T, _lib.stream_ptr()
    if c.entry == "cls":
        d = _dbg()
        rc = d.wise_debug_attention_cls_bf16(qkv.data_ptr(), B, T, H, o.data_ptr(), st)
        assert rc == 0, d.wise_last_error().decode()
        return
    lib = _lib.lib()
    if c.entry == "plain":
        rc = lib.wise_attention_bf16(qkv.data_ptr(), B, T, H, o.data_ptr(), st)
    elif c.entry == "dh":
        rc = lib.wise_attention_dh_bf16(qkv.data_ptr(), B, T, H, c.dh, o.data_ptr(), st)
    elif c.entry == "causal":
        rc = lib.wise_attention_causal_bf16(qkv.data_ptr(), B, T, H, o.data_ptr(), st)
    else:
        assert c.entry == "lens" and len(c.lens) == B
        lens = torch.tensor(c.lens, dtype=torch.int32, device="cuda")
        rc = lib.wise_attention_lens_bf16(qkv.data_ptr(), B, T, H, lens.data_ptr(), o.data_ptr(), st)
    _lib.check(rc, ac.ENTRY_POINT[c.entry])


@pytest.mark.parametrize("c", ac.CASES, ids=[ac.case_id(c) for c in ac.CASES])
def test_attention_exact(c):
    """one entry point, one family, one sequence length: every (B, H) of the case"""
    for B, H in c.sizes:
        qkv, exp = ac.build_case(c, B, H)
        rows = B if c.entry == "cls" else B * c.T
        what = f"{ac.ENTRY_POINT[c.entry]} {c.family} B={B} T={c.T} H={H} dh={c.dh} attention_kernel<{ac.instantiation(c.entry, c.T, c.dh)}>" \
               + (f" lens={c.lens}" if c.lens else "")
        out = _Guarded(rows, H * c.dh)
        _launch(c, B, H, _dev(qkv), out.body)
        torch.cuda.synchronize()
        _assert_bits(out, exp, what, 1 if c.entry == "cls" else c.T, c.dh)


@pytest.mark.parametrize("c", ac.SWIN_CASES, ids=[ac.swin_case_id(c) for c in ac.SWIN_CASES])
def test_swin_attention_exact(c):
    """swin_attention_kernel as htsat_forward_impl launches it: B = 1 and 3"""
    d = _dbg()
    for B in ac.SWIN_BATCHES:
        qkv, relb, exp = ac.build_swin(c.family, B, c.H, c.C, c.shift, ac.swin_case_seed(c))
        out = _Guarded(B * c.H * c.H, c.C)
        qd, rd = _dev(qkv), torch.from_numpy(relb).cuda()
        rc = d.wise_debug_swin_attention(qd.data_ptr(), B, c.H, c.C, c.shift, rd.data_ptr(), out.body.data_ptr(), _lib.stream_ptr())
        assert rc == 0, d.wise_last_error().decode()
        torch.cuda.synchronize()
        _assert_bits(out, exp, f"wise_debug_swin_attention {c.family} B={B} H={c.H} C={c.C} shift={c.shift}", c.H * c.H, 24)


def test_swin_debug_entry_refuses_other_shapes():
    d = _dbg()
    t = torch.zeros(64, device="cuda")
    p = t.data_ptr()
    assert d.wise_debug_swin_attention(p, 1, 12, 96, 0, p, p, _lib.stream_ptr()) != 0
    assert d.wise_debug_swin_attention(p, 1, 8, 100, 0, p, p, _lib.stream_ptr()) != 0
    assert d.wise_debug_swin_attention(p, 1, 8, 96, 2, p, p, _lib.stream_ptr()) != 0
    assert b"debug_swin_attention" in d.wise_last_error()

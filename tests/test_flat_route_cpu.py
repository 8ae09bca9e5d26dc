"""The search route of the flat codec indexes (wise_amd/index/flat_common.py: FlatCodecIndex, FlatIndexBase._exact_scan) and the
fp32 staging generator, driven on the CPU against a library stand-in that records every call: which entry point each search
takes, and its argument tuple position by position against include/wise_hip.h restated here by hand per type.  An argument in
the wrong place in one of these ctypes calls is a GPU fault, so it is caught here."""
import numpy as np
import pytest
import torch

from wise_amd import _lib
from wise_amd.index import flat_common, flat_ip
from wise_amd.index.flat_ip import FlatIPIndex
from wise_amd.index.flat_l2 import FlatL2Index
from wise_amd.index.flat_pq import FlatPQIPIndex
from wise_amd.index.flat_sq import FlatSQ8IPIndex, FlatSQfp16IPIndex, FlatSQfp16L2Index

N, DIM, K, ST, ID_BASE = 4096, 256, 10, 0x5EED, 7          # the smallest shape the batched route accepts


class RecordingLib:
    """Every entry point records (name, args) and returns 0; a *_workspace_bytes function returns what `bytes_of` holds for it."""

    def __init__(self):
        self.calls, self.bytes_of = [], {}

    def __getattr__(self, name):
        if name.endswith("_workspace_bytes"):
            return lambda *args: self.bytes_of.get(name, 4096)

        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry

    def names(self):
        return [name for name, _ in self.calls]


class Resolved:
    """what resolve_for returns: the positions a selector leaves, and its bitmap"""

    def __init__(self):
        self.pos = torch.arange(0, N, 2, dtype=torch.int64)
        self.bitmap = torch.zeros(N // 32, dtype=torch.int32)

    def positions(self):
        return self.pos


@pytest.fixture
def rec(monkeypatch):
    rec = RecordingLib()
    rec.resolved = Resolved()
    rec.mem_free, rec.mem_asked = 1 << 40, 0

    def mem_get_info(device=None):
        rec.mem_asked += 1
        return rec.mem_free, 1 << 40
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: ST)
    monkeypatch.setattr(flat_common, "resolve_for", lambda index, sel: rec.resolved)
    monkeypatch.setattr(flat_ip, "resolve_for", lambda index, sel: rec.resolved)
    monkeypatch.setattr(torch.cuda, "mem_get_info", mem_get_info)
    return rec


def _ids():
    return torch.arange(N, dtype=torch.int64) * 3


def _l2():
    return FlatL2Index(DIM, device="cpu").adopt(torch.zeros(N, DIM), _ids(), ID_BASE)


def _sq16():
    return FlatSQfp16IPIndex(DIM, device="cpu").adopt(torch.zeros(N, DIM, dtype=torch.float16), _ids(), ID_BASE)


def _sq16_l2():
    return FlatSQfp16L2Index(DIM, device="cpu").adopt(torch.zeros(N, DIM, dtype=torch.float16), _ids(), ID_BASE)


def _sq8():
    idx = FlatSQ8IPIndex(DIM, device="cpu")
    idx.set_trained(torch.zeros(DIM), torch.ones(DIM))
    return idx.adopt(torch.zeros(N, DIM, dtype=torch.uint8), _ids(), ID_BASE)


def _ip():
    return FlatIPIndex(DIM, device="cpu", shadow=False).adopt(torch.zeros(N, DIM), _ids(), ID_BASE)


p = lambda t: t.data_ptr()
# Per type: the entry points (exact scan over all rows, over pos[], its workspace bytes; the batched search, its workspace bytes,
# the prepare call) and, BY HAND from include/wise_hip.h, what each call passes in front of `N, d`:
#   head      the exact scans and the batched search open with the rows, then — IndexSQ8bit only — trained
#   operands  what the batched search takes between that and N
#   prepared  the whole argument list of the prepare call
CASES = {
    "FlatL2Index": dict(
        make=_l2, topk="wise_l2_topk_f32", pos="wise_l2_topk_pos_f32", bytes="wise_l2_topk_workspace_bytes",
        batched="wise_l2_topk_batched", bbytes="wise_l2_topk_batched_workspace_bytes", prepare="wise_l2_prepare",
        head=lambda i: (p(i._X),),
        operands=lambda i: (p(i._Xb), p(i._half), p(i._norms)),
        prepared=lambda i: (p(i._X), N, DIM, p(i._Xb), p(i._half), p(i._norms), ST)),
    "FlatSQfp16IPIndex": dict(
        make=_sq16, topk="wise_ipsq16_topk", pos="wise_ipsq16_topk_pos", bytes="wise_ipsqfp16_topk_workspace_bytes",
        batched="wise_ipsq16_topk_batched", bbytes="wise_ipsqfp16_topk_batched_workspace_bytes", prepare="wise_ipsq16_prepare",
        head=lambda i: (p(i._H),),
        operands=lambda i: (p(i._norms),),
        prepared=lambda i: (p(i._H), N, DIM, p(i._norms), ST)),
    "FlatSQfp16L2Index": dict(
        make=_sq16_l2, topk="wise_l2sq16_topk", pos="wise_l2sq16_topk_pos", bytes="wise_l2sqfp16_topk_workspace_bytes",
        batched="wise_l2sq16_topk_batched", bbytes="wise_l2sqfp16_topk_batched_workspace_bytes", prepare="wise_l2sq16_prepare",
        head=lambda i: (p(i._H),),
        operands=lambda i: (p(i._half), p(i._norms)),
        prepared=lambda i: (p(i._H), N, DIM, p(i._half), p(i._norms), ST)),
    "FlatSQ8IPIndex": dict(
        make=_sq8, topk="wise_ipsq8_topk", pos="wise_ipsq8_topk_pos", bytes="wise_ipsq8_topk_workspace_bytes",
        batched="wise_ipsq8_topk_batched", bbytes="wise_ipsq8_topk_batched_workspace_bytes", prepare="wise_ipsq8_prepare",
        head=lambda i: (p(i._codes_t), p(i._trained)),
        operands=lambda i: (p(i._norms),),
        prepared=lambda i: (p(i._codes_t), N, DIM, p(i._norms), ST)),
    "FlatIPIndex": dict(
        make=_ip, topk="wise_ip_topk_f32", pos="wise_ip_topk_pos_f32", bytes="wise_ip_topk_workspace_bytes",
        batched=None, bbytes=None, prepare=None,
        head=lambda i: (p(i._X),)),
}
CODECS = [name for name, case in CASES.items() if case["batched"]]


def _queries(nq):
    return torch.zeros(nq, DIM)


def _tail(idx, q, D, I, ws):
    """what every search entry point ends with: Q, nq, k, ids, id_base, outD, outI, [counters,] workspace, its bytes, the stream"""
    return (p(q), q.shape[0], K, p(idx._ids), ID_BASE, p(D), p(I)), (p(ws), ws.numel(), ST)


def _expect_exact(case, idx, q, D, I, pos=None):
    a, b = _tail(idx, q, D, I, idx._ws)
    over = () if pos is None else (p(pos), pos.numel())
    return (case["pos" if pos is not None else "topk"], case["head"](idx) + (N, DIM) + over + a + b)


def _expect_batched(case, idx, q, D, I):
    a, b = _tail(idx, q, D, I, idx._bws)
    return (case["batched"], case["head"](idx) + case["operands"](idx) + (N, DIM) + a + (p(idx._counters),) + b)


def _search(rec, idx, nq, sel=None):
    """one search_device: (the calls it made, q, D, I)"""
    before = len(rec.calls)
    q = _queries(nq)
    D, I = idx.search_device(q, K) if sel is None else idx.search_device(q, K, sel=sel)
    assert D.shape == (nq, K) and D.dtype == torch.float32 and I.shape == (nq, K) and I.dtype == torch.int64
    calls = rec.calls[before:]
    for name, args in calls:
        assert len(args) == len(_lib.SIGNATURES[name][1]), name
    return calls, q, D, I


@pytest.mark.parametrize("name", list(CASES))
def test_every_route_calls_its_entry_point_with_its_arguments(rec, name):
    case = CASES[name]
    idx = case["make"]()
    idx.BATCH_MIN_ROWS = N
    batched = case["batched"] is not None
    # under a selector: the exact scan over its positions, whatever the batch
    calls, q, D, I = _search(rec, idx, 3, sel=object())
    assert calls == [_expect_exact(case, idx, q, D, I, rec.resolved.pos)]
    # 8 queries: the batched search where the type has one, behind ONE prepare call
    calls, q, D, I = _search(rec, idx, 8)
    if batched:
        assert calls == [(case["prepare"], case["prepared"](idx)), _expect_batched(case, idx, q, D, I)]
        assert idx._bws.numel() == 4096
    else:
        assert calls == [_expect_exact(case, idx, q, D, I)]
    # 7 queries: the exact scan over all rows
    calls, q, D, I = _search(rec, idx, 7)
    assert calls == [_expect_exact(case, idx, q, D, I)]
    if not batched:
        return
    # a second batch finds the derived arrays in place ...
    calls, q, D, I = _search(rec, idx, 8)
    assert calls == [_expect_batched(case, idx, q, D, I)]
    assert rec.names().count(case["prepare"]) == 1
    assert idx.batched_counts() == (0, 0)                          # the stand-in counts nothing; the tensor is there and read
    # ... and builds them again once the rows changed
    held = idx._norms
    idx._rows_changed()
    assert idx._norms is None and getattr(idx, "_half", None) is None and getattr(idx, "_Xb", None) is None
    calls, q, D, I = _search(rec, idx, 8)
    assert calls == [(case["prepare"], case["prepared"](idx)), _expect_batched(case, idx, q, D, I)]
    assert idx._norms is not None and idx._norms is not held


@pytest.mark.parametrize("name", CODECS)
def test_batched_route_needs_its_floor_and_a_served_shape(rec, name):
    case = CASES[name]
    idx = case["make"]()
    calls, q, D, I = _search(rec, idx, 8)                          # the class's BATCH_MIN_ROWS: 4096 rows are too few
    assert calls == [_expect_exact(case, idx, q, D, I)]
    idx.BATCH_MIN_ROWS = N
    idx.BATCH_MIN_QUERIES = 9
    calls, q, D, I = _search(rec, idx, 8)
    assert calls == [_expect_exact(case, idx, q, D, I)]
    idx.BATCH_MIN_QUERIES = 8
    rec.bytes_of[case["bbytes"]] = 0                               # the batched search does not serve the shape
    calls, q, D, I = _search(rec, idx, 8)
    assert calls == [_expect_exact(case, idx, q, D, I)]
    assert idx._norms is None and idx._bws is None and idx._counters is None and idx.batched_counts() == (0, 0)


@pytest.mark.parametrize("name", list(CASES))
def test_unsupported_shape_and_empty_batch(rec, name):
    case = CASES[name]
    idx = case["make"]()
    rec.bytes_of[case["bytes"]] = 0
    with pytest.raises(ValueError, match=f"^search: unsupported shape N={N} d={DIM} nq=7 k={K}$"):
        idx.search_device(_queries(7), K)
    with pytest.raises(ValueError, match=f"^search: unsupported shape N={N} d={DIM} nq=3 k={K}$"):
        idx.search_device(_queries(3), K, sel=object())
    D, I = idx.search_device(_queries(0), K)
    assert D.shape == (0, K) and D.dtype == torch.float32 and I.shape == (0, K) and I.dtype == torch.int64
    D, I = idx.search_device(_queries(0), K, sel=object())
    assert D.shape == (0, K) and I.shape == (0, K)
    assert rec.calls == []
    with pytest.raises(ValueError, match=r"^search: expected \[nq,256\]"):
        idx.search_device(torch.zeros(2, DIM + 1), K)


def test_flat_l2_without_room_switches_its_batched_route_off(rec):
    case = CASES["FlatL2Index"]
    idx = case["make"]()
    idx.BATCH_MIN_ROWS = N
    rec.mem_free = 0
    calls, q, D, I = _search(rec, idx, 8)
    assert calls == [_expect_exact(case, idx, q, D, I)]
    assert rec.mem_asked == 1 and idx._Xb is None and idx.BATCH_MIN_ROWS == 1 << 62
    assert FlatL2Index.BATCH_MIN_ROWS == 1 << 18                   # this index alone
    rec.mem_free = 1 << 40
    calls, q, D, I = _search(rec, idx, 8)
    assert calls == [_expect_exact(case, idx, q, D, I)]
    assert rec.mem_asked == 1


def test_sq8_search_needs_training(rec):
    with pytest.raises(RuntimeError, match="IndexSQ8bit: search before train"):
        FlatSQ8IPIndex(DIM, device="cpu").search_device(_queries(1), K)


# ---- the staging generator
STAGERS = {"FlatSQfp16IPIndex": lambda: FlatSQfp16IPIndex(16, device="cpu"), "FlatSQfp16L2Index": lambda: FlatSQfp16L2Index(16, device="cpu"),
           "FlatSQ8IPIndex": lambda: FlatSQ8IPIndex(16, device="cpu"), "FlatPQIPIndex": lambda: FlatPQIPIndex(16, 4, device="cpu")}


@pytest.mark.parametrize("name", list(STAGERS))
def test_staged_copies_and_converts_what_is_not_fp32_device_contiguous(name):
    idx = STAGERS[name]()
    idx.ENCODE_BYTES = 4 * 16 * 300
    x = np.random.default_rng(5).standard_normal((700, 16))
    want = x.astype(np.float32)
    starts, buffers = [], set()
    for s, part in idx._staged(torch.from_numpy(x)):
        starts.append(s)
        buffers.add(part.data_ptr())
        assert part.dtype == torch.float32 and part.is_contiguous() and part.device.type == idx.device.type
        assert np.array_equal(part.numpy(), want[s:s + 300])
    assert starts == [0, 300, 600] and len(buffers) == 1          # ONE staging buffer
    # rows that need no copy are yielded as views
    t = torch.from_numpy(want)
    parts = list(idx._staged(t))
    assert [s for s, _ in parts] == [0, 300, 600]
    for s, part in parts:
        assert part.data_ptr() == t[s:].data_ptr() and part.shape == (min(300, 700 - s), 16)
    # a non-contiguous chunk is copied
    (s, part), = idx._staged(torch.from_numpy(want[:200].T.copy()).T)
    assert s == 0 and part.is_contiguous() and np.array_equal(part.numpy(), want[:200])
    assert list(idx._staged(t[:0])) == []


def test_sqfp16_fill_encodes_chunk_by_chunk_without_converting_the_whole_input(rec):
    idx = FlatSQfp16IPIndex(16, device="cpu")
    idx.ENCODE_BYTES = 4 * 16 * 300
    x = torch.from_numpy(np.random.default_rng(6).standard_normal((700, 16)))      # float64
    dst = torch.empty(700, 16, dtype=torch.float16)
    idx._fill(dst, x)
    assert rec.names() == ["wise_sq16_encode"] * 3
    stage = rec.calls[0][1][0]
    for (name, args), s in zip(rec.calls, (0, 300, 600)):
        assert args == (stage, min(300, 700 - s), 16, dst[s:].data_ptr(), ST)
        assert len(args) == len(_lib.SIGNATURES[name][1])

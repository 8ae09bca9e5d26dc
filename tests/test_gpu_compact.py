"""-m gpu: the compaction kernels behind remove_ids (csrc/compact.hip) through the C ABI, bit for bit against the numpy
restatement (tests/mutate_ref.py).  The bytes behind the kept rows are unspecified and never compared; guard bytes behind
the array and behind the scratch are."""
import numpy as np
import pytest
import torch

import mutate_ref
from wise_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 64
SIZES = [0, 1, 31, 32, 33, 2047, 2048, 2049, 5000]
WIDTHS = [4, 8, 12, 16, 48, 64, 2048, 4096]
BIG = 1 << 26          # a scratch larger than every array here


def masks(N, rng, run):
    """name -> bool [N], True = the row stays.  run: the length of the removed run of the last mask."""
    out = {"all": np.ones(N, bool), "none": np.zeros(N, bool)}
    if N:
        first = np.ones(N, bool); first[0] = False
        last = np.ones(N, bool); last[N - 1] = False
        out.update(first_removed=first, last_removed=last, alternating=(np.arange(N) & 1).astype(bool),
                   sparse=rng.random(N) < 0.01, dense=rng.random(N) < 0.99)
        hole = np.ones(N, bool)
        a = N // 5
        hole[a:a + min(run, N - a)] = False
        out["long_run"] = hole
    return out


def keep_words(mask, garbage_tail=False):
    w = mutate_ref.bitmap(mask)
    n = mask.shape[0]
    if garbage_tail and n & 31:
        w[-1] |= np.uint32((0xFFFFFFFF << (n & 31)) & 0xFFFFFFFF)       # every bit past N set
    return torch.from_numpy(w.view(np.int32)).cuda() if w.size else torch.zeros(1, dtype=torch.int32, device="cuda")


def gpu_plan(keep, N):
    lib, st = _lib.lib(), _lib.stream_ptr()
    entries = int(lib.wise_compact_plan_entries(N))
    assert entries == (N + 2047) // 2048 + 1
    plan = torch.full((entries + 1,), -7, dtype=torch.int64, device="cuda")
    count = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    _lib.check(lib.wise_compact_plan(keep.data_ptr(), N, plan.data_ptr(), count.data_ptr(), st), "wise_compact_plan")
    assert int(plan[entries]) == -7 and int(count[1]) == -7
    return plan[:entries], count


def gpu_compact(rows, mask, scratch_bytes, garbage_tail=False, offset=0):
    """rows [N, width] uint8 -> (the first kept rows of the array after wise_compact_rows, the whole buffer's bytes)."""
    lib, st = _lib.lib(), _lib.stream_ptr()
    N, width = rows.shape
    keep = keep_words(mask, garbage_tail)
    plan, count = gpu_plan(keep, N)
    kept = int(mask.sum())
    assert int(count[0]) == kept
    seg = np.minimum(np.arange(plan.numel(), dtype=np.int64) * 2048, N)
    assert np.array_equal(plan.cpu().numpy(), mutate_ref.rank(mask, seg))
    buf = torch.full((offset + N * width + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[offset:offset + N * width] = torch.from_numpy(rows.reshape(-1)).cuda()
    scratch = torch.full((scratch_bytes + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    _lib.check(lib.wise_compact_rows(buf.data_ptr() + offset, N, width, keep.data_ptr(), plan.data_ptr(), scratch.data_ptr(),
                                     scratch_bytes, st), "wise_compact_rows")
    out = buf.cpu().numpy()
    assert (out[:offset] == 0xA5).all() and (out[offset + N * width:] == 0xA5).all()      # nothing written outside the array
    assert (scratch[scratch_bytes:] == 0x5A).all()                                         # ... or outside the scratch
    return out[offset:offset + kept * width].reshape(kept, width), out


def make_rows(N, width, rng):
    return rng.integers(0, 256, size=(N, width), dtype=np.uint8)


@pytest.mark.parametrize("width", WIDTHS)
def test_main_grid_equals_the_restatement(width):
    rng = np.random.default_rng(width)
    for N in SIZES:
        rows = make_rows(N, width, rng)
        for name, mask in masks(N, rng, run=N // 2).items():
            got, _ = gpu_compact(rows, mask, BIG)
            assert np.array_equal(got, mutate_ref.compact(rows, mask)), (width, N, name)


@pytest.mark.parametrize("width", [4, 12, 64, 2048])
@pytest.mark.parametrize("scratch_rows", [1, 7])
def test_small_scratch_forces_many_chunks(width, scratch_rows):
    """A scratch of one row and of seven rows: every chunk boundary falls inside a bitmap word, chunks whose destinations
    overlap their sources, chunks written in place, and a removed run much longer than a chunk."""
    rng = np.random.default_rng(100 + width + scratch_rows)
    for N in (1, 33, 2049) if width != 64 else (1, 33, 2049, 5000):      # 5000 x 64 B under 7 rows: 715 chunks
        rows = make_rows(N, width, rng)
        for name, mask in masks(N, rng, run=max(N // 3, 1)).items():
            got, _ = gpu_compact(rows, mask, scratch_rows * width)
            assert np.array_equal(got, mutate_ref.compact(rows, mask)), (width, N, scratch_rows, name)


def test_scratch_of_a_few_segments():
    """More than 2048 rows fit: chunks are whole segments (here 4096 rows of a 10000-row array)."""
    rng = np.random.default_rng(5)
    N, width = 10000, 16
    rows = make_rows(N, width, rng)
    for name, mask in masks(N, rng, run=5000).items():
        got, _ = gpu_compact(rows, mask, 5000 * width)
        assert np.array_equal(got, mutate_ref.compact(rows, mask)), name


@pytest.mark.parametrize("N", [1, 31, 33, 2047, 2049, 5000])
def test_garbage_tail_bits_are_ignored(N):
    rng = np.random.default_rng(N)
    rows = make_rows(N, 8, rng)
    for name, mask in masks(N, rng, run=N // 2).items():
        got, _ = gpu_compact(rows, mask, 7 * 8, garbage_tail=True)
        assert np.array_equal(got, mutate_ref.compact(rows, mask)), name


@pytest.mark.parametrize("width", [4, 12])
def test_base_aligned_to_4_bytes_only(width):
    rng = np.random.default_rng(width)
    for N in (33, 2049, 5000):
        rows = make_rows(N, width, rng)
        for name, mask in masks(N, rng, run=N // 2).items():
            for scratch in (7 * width, BIG):
                got, _ = gpu_compact(rows, mask, scratch, offset=4)
                assert np.array_equal(got, mutate_ref.compact(rows, mask)), (N, name, scratch)


def test_same_call_twice_gives_the_same_bytes():
    rng = np.random.default_rng(9)
    N, width = 5000, 48
    rows = make_rows(N, width, rng)
    mask = rng.random(N) < 0.6
    for scratch in (7 * width, 3000 * width, BIG):
        a = gpu_compact(rows, mask, scratch)[1]
        b = gpu_compact(rows, mask, scratch)[1]
        assert np.array_equal(a, b)                    # the whole buffer, the unspecified tail included


def gpu_rank(mask, pos, garbage_tail=False):
    lib, st = _lib.lib(), _lib.stream_ptr()
    N = mask.shape[0]
    keep = keep_words(mask, garbage_tail)
    plan, _ = gpu_plan(keep, N)
    p = torch.from_numpy(np.asarray(pos, dtype=np.int64)).cuda()
    out = torch.full((p.numel() + 1,), -7, dtype=torch.int64, device="cuda")
    _lib.check(lib.wise_compact_rank(keep.data_ptr(), N, plan.data_ptr(), p.data_ptr(), p.numel(), out.data_ptr(), st),
               "wise_compact_rank")
    assert int(out[-1]) == -7
    return out[:-1].cpu().numpy()


@pytest.mark.parametrize("N", [0, 1, 33, 2048, 4096, 5000, 6144])
def test_rank_equals_the_restatement(N):
    rng = np.random.default_rng(N)
    edges = [p for s in range(0, N + 2049, 2048) for p in (s - 1, s, s + 1)] + [0, N, N - 1, N // 2, 31, 32, 33]
    pos = np.array(sorted({p for p in edges if 0 <= p <= N}), dtype=np.int64)
    # a sorted list_off with empty lists: repeated offsets, lists that end at 0 and at N
    off = np.sort(np.concatenate([[0, 0, N, N], rng.integers(0, N + 1, size=20), rng.integers(0, N + 1, size=5).repeat(2)]))
    for name, mask in masks(N, rng, run=N // 2).items():
        for p in (pos, off):
            assert np.array_equal(gpu_rank(mask, p, garbage_tail=True), mutate_ref.rank(mask, p)), (N, name)
        assert np.array_equal(gpu_rank(mask, off), mutate_ref.new_list_off(off, mask))


def test_captured_into_a_graph():
    """plan, rank and rows neither allocate nor read back: one capture, replayed on fresh contents."""
    lib = _lib.lib()
    rng = np.random.default_rng(3)
    N, width = 5000, 64
    rows = make_rows(N, width, rng)
    mask = rng.random(N) < 0.5
    keep = keep_words(mask)
    data = torch.zeros(N * width, dtype=torch.uint8, device="cuda")
    plan = torch.zeros(int(lib.wise_compact_plan_entries(N)), dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    off = torch.from_numpy(np.array([0, 100, 100, 2500, N], dtype=np.int64)).cuda()
    new_off = torch.zeros_like(off)
    scratch = torch.empty(1000 * width, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = _lib.stream_ptr()
        _lib.check(lib.wise_compact_plan(keep.data_ptr(), N, plan.data_ptr(), count.data_ptr(), st))
        _lib.check(lib.wise_compact_rank(keep.data_ptr(), N, plan.data_ptr(), off.data_ptr(), off.numel(), new_off.data_ptr(), st))
        _lib.check(lib.wise_compact_rows(data.data_ptr(), N, width, keep.data_ptr(), plan.data_ptr(), scratch.data_ptr(),
                                         scratch.numel(), st))
    data.copy_(torch.from_numpy(rows.reshape(-1)).cuda())
    g.replay()
    torch.cuda.synchronize()
    kept = int(mask.sum())
    assert int(count[0]) == kept
    assert np.array_equal(new_off.cpu().numpy(), mutate_ref.new_list_off(off.cpu().numpy(), mask))
    assert np.array_equal(data[:kept * width].cpu().numpy().reshape(kept, width), mutate_ref.compact(rows, mask))


def test_invalid_arguments_are_refused():
    lib, st = _lib.lib(), _lib.stream_ptr()
    t = torch.zeros(1024, dtype=torch.int64, device="cuda")
    p = t.data_ptr()

    def refused(rc):
        assert rc == -1 and lib.wise_last_error()      # WISE_E_INVALID with a text

    refused(lib.wise_compact_plan(p, -1, p, p, st))
    refused(lib.wise_compact_plan(p, 1 << 32, p, p, st))
    refused(lib.wise_compact_plan(0, 10, p, p, st))
    refused(lib.wise_compact_plan(p, 10, 0, p, st))
    refused(lib.wise_compact_plan(p, 10, p, 0, st))
    refused(lib.wise_compact_rank(p, -1, p, p, 1, p, st))
    refused(lib.wise_compact_rank(p, 10, 0, p, 1, p, st))
    refused(lib.wise_compact_rank(p, 10, p, 0, 1, p, st))
    refused(lib.wise_compact_rank(p, 10, p, p, -1, p, st))
    refused(lib.wise_compact_rows(p, -1, 8, p, p, p, 64, st))
    refused(lib.wise_compact_rows(p, 10, 0, p, p, p, 64, st))
    refused(lib.wise_compact_rows(p, 10, 1 << 20, p, p, p, 1 << 21, st))
    refused(lib.wise_compact_rows(p, 10, 8, p, p, p, 7, st))          # a scratch that holds no row
    refused(lib.wise_compact_rows(0, 10, 8, p, p, p, 64, st))
    refused(lib.wise_compact_rows(p, 10, 8, 0, p, p, 64, st))
    refused(lib.wise_compact_rows(p, 10, 8, p, 0, p, 64, st))
    refused(lib.wise_compact_rows(p, 10, 8, p, p, 0, 64, st))
    assert lib.wise_compact_plan_entries(-1) == 0
    assert lib.wise_compact_rows(0, 0, 8, 0, 0, 0, 0, st) == 0        # N = 0: nothing to do, nothing needed
    torch.cuda.synchronize()
    assert (t == 0).all()

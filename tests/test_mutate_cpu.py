"""No GPU: the compaction entry points are declared, bound and exported under ABI 5; plan_update against the restatement by
sets (tests/mutate_ref.py); the refusals of remove_ids / update_index that need no device."""
import re
from pathlib import Path

import numpy as np
import pytest

import mutate_ref

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("wise_compact_plan_entries", "wise_compact_plan", "wise_compact_rank", "wise_compact_rows")


def test_symbols_declared_and_bound():
    from wise_amd import _lib, build
    declared = build.declared_symbols()
    for name in SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
    assert set(_lib.SIGNATURES) == set(declared)
    assert "compact.hip" in build.HIP_SOURCES and (build.CSRC / "compact.hip").exists()


def test_abi_stays_5():
    header = (ROOT / "include" / "wise_hip.h").read_text()
    intro = header[header.index("/* ABI version of this header"):header.index("int wise_abi_version(void);")]
    assert "The version is 5." in intro and "wise_compact_rows" in intro and not re.search(r"\b6:", intro)
    assert "(ABI 5, additive) remove_ids" in header
    assert "wise_abi_version(void) { return 5; }" in (ROOT / "wise_amd" / "csrc" / "common.hip").read_text()


def test_library_exports_and_argument_rules():
    import subprocess
    from wise_amd import _lib, build
    if not _lib.LIB_PATH.exists():
        pytest.skip("library not built")
    lib = _lib.load()
    assert lib.wise_abi_version() == 5
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert exported == set(build.declared_symbols())                   # exports == header
    assert [lib.wise_compact_plan_entries(n) for n in (0, 1, 2048, 2049, 10_000_000)] == [1, 2, 2, 3, 4884]
    assert lib.wise_compact_plan_entries(-1) == 0 and lib.wise_compact_plan_entries(0xFFFFFFFF) == 0
    # argument checks come before any launch
    assert lib.wise_compact_plan(16, -1, 16, 16, 0) == -1 and b"compact_plan" in lib.wise_last_error()
    assert lib.wise_compact_rank(16, 10, 0, 16, 1, 16, 0) == -1 and b"compact_rank" in lib.wise_last_error()
    assert lib.wise_compact_rows(16, 10, 0, 16, 16, 16, 64, 0) == -1 and b"width_bytes" in lib.wise_last_error()
    assert lib.wise_compact_rows(16, 10, 8, 16, 16, 16, 7, 0) == -1 and b"scratch" in lib.wise_last_error()
    assert lib.wise_compact_rows(0, 10, 8, 16, 16, 16, 64, 0) == -1 and b"null" in lib.wise_last_error()


def test_mutate_ref_rules():
    mask = np.array([1, 0, 1, 1, 0, 0, 1], dtype=bool)
    a = np.arange(14).reshape(7, 2)
    assert mutate_ref.compact(a, mask).tolist() == [[0, 1], [4, 5], [6, 7], [12, 13]]
    assert mutate_ref.rank(mask, [0, 1, 2, 7]).tolist() == [0, 1, 1, 4]
    assert mutate_ref.new_list_off(np.array([0, 0, 3, 3, 7]), mask).tolist() == [0, 0, 2, 2, 4]
    assert mutate_ref.bitmap(mask).tolist() == [0b1001101]
    assert mutate_ref.bitmap(np.ones(33, bool)).tolist() == [0xFFFFFFFF, 1] and mutate_ref.bitmap(np.zeros(0, bool)).size == 0


CASES = {
    "disjoint": ([5, 3, 9], [10, 2, 7]),
    "identical": ([4, 8, 1], [1, 4, 8]),
    "empty_index": ([], [3, 1, 2]),
    "empty_store": ([3, 1, 2], []),
    "both_empty": ([], []),
    "both_ways": ([10, 20, 30, 40, 50], [60, 50, 5, 20, 70, 10]),      # 30 and 40 go; 60, 5 and 70 come, in store order
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_update_equals_the_restatement(name):
    from wise_amd.index.mutate import plan_update
    index_ids, store_ids = (np.array(a, dtype=np.int64) for a in CASES[name])
    remove, add = plan_update(index_ids, store_ids)
    want_remove, want_add = mutate_ref.plan_update(index_ids, store_ids)
    assert remove.dtype == np.int64 and add.dtype == bool and add.shape == store_ids.shape
    assert np.array_equal(remove, want_remove) and np.array_equal(add, want_add)


def test_plan_update_keeps_store_order_and_refuses_duplicates():
    from wise_amd.index.mutate import plan_update
    rng = np.random.default_rng(2)
    universe = rng.permutation(5000).astype(np.int64) * 7 - 300          # negative ids too
    index_ids, store_ids = universe[:3000], rng.permutation(universe[1000:])
    remove, add = plan_update(index_ids, store_ids)
    want_remove, want_add = mutate_ref.plan_update(index_ids, store_ids)
    assert np.array_equal(remove, want_remove) and np.array_equal(add, want_add)
    assert np.array_equal(np.sort(remove), np.sort(universe[:1000])) and int(add.sum()) == 2000
    new = set(universe[3000:].tolist())
    assert np.array_equal(store_ids[add], [i for i in store_ids if i in new])                        # store order kept
    with pytest.raises(ValueError, match="more than once"):
        plan_update([1, 2, 3], [4, 5, 4])
    with pytest.raises(ValueError, match="more than once"):
        plan_update([1, 2, 2], [4, 5])


def test_sharded_wrappers_refuse_remove_ids():
    from wise_amd.index.flat_ip import FlatIPIndex
    from wise_amd.index.ivf_flat import IVFFlatIPIndex
    from wise_amd.index.ivf_pq import IVFPQIPIndex, IVFPQRefineIPIndex
    from wise_amd.index.ivf_sq import IVFSQIPIndex
    from wise_amd.index.selector import IDSelectorRange
    from wise_amd.index import sharded
    wrapped = [sharded.ShardedFlatIPIndex(FlatIPIndex(16, device="cpu")),
               sharded.ShardedIVFFlatIPIndex(IVFFlatIPIndex(16, 4, device="cpu")),
               sharded.ShardedIVFPQIPIndex(IVFPQIPIndex(32, 4, 8, device="cpu")),
               sharded.ShardedIVFPQRefineIPIndex(IVFPQRefineIPIndex(32, 4, 8, 8, device="cpu")),
               sharded.ShardedIVFSQIPIndex(IVFSQIPIndex(32, 4, device="cpu"))]
    for sh in wrapped:
        with pytest.raises(NotImplementedError, match="collective removal is not built"):
            sh.remove_ids(IDSelectorRange(0, 10))
        with pytest.raises(NotImplementedError, match="collective removal is not built"):
            sh.remove_ids(np.array([1, 2, 3]))
    # the refusals that were there stay
    with pytest.raises(NotImplementedError, match="no selector"):
        wrapped[0].search_device(None, 5, sel=IDSelectorRange(0, 10))
    # every index class has the method and the class-level default workspace of 64 MiB
    for cls in (FlatIPIndex, IVFFlatIPIndex, IVFPQIPIndex, IVFPQRefineIPIndex, IVFSQIPIndex):
        assert callable(cls.remove_ids) and cls.REMOVE_SCRATCH_BYTES == 64 << 20


def test_update_index_refusals(tmp_path):
    from wise_amd.index.feature_search_index import FeatureSearchIndex
    fdir, idir = tmp_path / "features", tmp_path / "index"
    fdir.mkdir()
    idir.mkdir()
    si = FeatureSearchIndex("video", "mlfoundations/open_clip/ViT-B-32/seeded-0", {"features_dir": fdir, "index_dir": idir})
    for index_type in ("IndexFlatIP", "IndexIVFFlat", "IndexIVFSQ8", "IndexIVFPQ16R8"):
        with pytest.raises(FileNotFoundError, match="create_index"):
            si.update_index(index_type)
    with pytest.raises(NotImplementedError) as update_err:
        si.update_index("IndexHNSW")
    with pytest.raises(NotImplementedError) as create_err:
        si.create_index("IndexHNSW")
    assert str(update_err.value) == str(create_err.value)              # the existing message, unchanged
    assert not si.is_index_loaded() and not hasattr(si, "feature_extractor")

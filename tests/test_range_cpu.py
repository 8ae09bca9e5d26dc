"""No GPU: the range_search entry points are declared, bound and exported under ABI 5; tests/range_ref.py's own rules; the
parameter objects and the refusals that need no device."""
import re
from pathlib import Path

import numpy as np
import pytest

import range_ref as rr

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("wise_ip_range_workspace_bytes", "wise_ip_range_count_f32", "wise_ip_range_fill_f32",
           "wise_ivf_range_workspace_bytes", "wise_ivf_range_count_f32", "wise_ivf_range_fill_f32",
           "wise_ivfsq_range_workspace_bytes", "wise_ivfsq_range_count", "wise_ivfsq_range_fill")


def test_symbols_declared_and_bound():
    from wise_amd import _lib, build
    declared = build.declared_symbols()
    for name in SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
    # a count takes the radius as a C float, a fill the same list plus lims / outD / outI
    import ctypes as C
    for name in SYMBOLS:
        if "workspace" not in name:
            assert C.c_float in _lib.SIGNATURES[name][1] and _lib.SIGNATURES[name][0] is C.c_int, name
    assert set(_lib.SIGNATURES) == set(declared)


def test_abi_stays_5():
    header = (ROOT / "include" / "wise_hip.h").read_text()
    intro = header[header.index("/* ABI version of this header"):header.index("int wise_abi_version(void);")]
    assert "The version is 5." in intro and "wise_ivfsq_range_*" in intro and not re.search(r"\b6:", intro)
    assert "wise_abi_version(void) { return 5; }" in (ROOT / "wise_amd" / "csrc" / "common.hip").read_text()
    assert "(ABI 5, additive) range_search" in header


def test_library_exports_and_workspace_rules():
    from wise_amd import _lib
    if not _lib.LIB_PATH.exists():
        pytest.skip("library not built")
    lib = _lib.load()
    assert lib.wise_abi_version() == 5
    assert lib.wise_ip_range_workspace_bytes(0, 16, 1) > 0             # an empty index still has counts to write
    assert lib.wise_ip_range_workspace_bytes(6000, 16, 5) >= 5 * (6000 // 8)
    for bad in ((-1, 16, 1), (100, 6, 1), (100, 2052, 1), (100, 16, 0), (100, 16, 65536), (0xFFFFFFFF, 16, 1)):
        assert lib.wise_ip_range_workspace_bytes(*bad) == 0, bad
    assert lib.wise_ivf_range_workspace_bytes(6000, 37, 5, 8) >= 5 * (6000 // 8)
    assert lib.wise_ivfsq_range_workspace_bytes(6000, 37, 5, 8) == lib.wise_ivf_range_workspace_bytes(6000, 37, 5, 8)
    for bad in ((6000, 0, 1, 1), (6000, 37, 0, 1), (6000, 37, 1, 0), (6000, 37, 1, 2049), (6000, 37, 65536, 1)):
        assert lib.wise_ivf_range_workspace_bytes(*bad) == 0 and lib.wise_ivfsq_range_workspace_bytes(*bad) == 0, bad
    # argument checks come before any launch: NaN / infinite radius, a short workspace
    for radius in (float("nan"), float("inf"), float("-inf")):
        assert lib.wise_ip_range_count_f32(16, 4, 16, 16, 1, radius, 0, 16, 16, 1 << 20, 0) == -1
        assert b"radius" in lib.wise_last_error()
    assert lib.wise_ip_range_count_f32(16, 4, 16, 16, 1, 0.5, 0, 16, 16, 8, 0) == -1 and b"workspace" in lib.wise_last_error()
    assert lib.wise_ivf_range_count_f32(16, 4, 16, 16, 2, 16, 1, 16, 1, 0.5, 0, 16, 16, 8, 0) == -1 and b"workspace" in lib.wise_last_error()
    assert lib.wise_ivfsq_range_count(16, 4, 16, 16, 2, 16, 16, 1, 16, 16, 1, 0.5, 0, 16, 16, 8, 0) == -1 and b"workspace" in lib.wise_last_error()
    assert lib.wise_ivfsq_range_count(16, 4, 24, 16, 2, 16, 16, 1, 16, 16, 1, 0.5, 0, 16, 16, 1 << 20, 0) == -1      # d % 16


def test_range_ref_rules():
    t = np.float32(0.25)
    up, down = np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0))
    assert rr.is_hit([up, t, down], 0.25).tolist() == [True, False, False]                       # strict
    D = np.array([0.9, up, t, t, down, rr.NEG, rr.NEG], dtype=np.float32)
    I = np.array([7, 3, 1, 2, 9, -1, -1])
    d, i = rr.prefix(D, I, 0.25)
    assert d.tolist() == [np.float32(0.9), up] and i.tolist() == [7, 3]
    d, i = rr.prefix(D, I, -3.4028235e38)                                                       # every real row, never the padding
    assert len(d) == 5 and i.tolist() == [7, 3, 1, 2, 9]
    assert len(rr.prefix(D, I, 0.9)[0]) == 0
    with pytest.raises(AssertionError):
        rr.prefix(D[:2], I[:2], 0.0)                                                            # full of hits: no oracle
    with pytest.raises(ValueError):
        rr.threshold32(float("nan"))
    # order: descending score, -0.0 below +0.0, ties by ascending position
    s = np.array([0.5, 0.5, -0.0, 0.0, 0.7], dtype=np.float32)
    p = np.array([9, 4, 1, 2, 30])
    assert rr.order(s, p).tolist() == [4, 1, 0, 3, 2]
    assert rr.in_order(s[rr.order(s, p)], p[rr.order(s, p)]) and not rr.in_order(s, p)


def test_thresholds_and_params():
    from wise_amd.index import range_search as rs
    from wise_amd.index.selector import IDSelectorRange, SearchParameters, SearchParametersIVF, unpack_params
    assert rs.check_threshold(0.28) == 0.28 and rs.check_threshold(-3.4028235e38) == -3.4028235e38
    assert rs.check_threshold(np.float32(0.5)) == 0.5 and rs.check_threshold(1) == 1.0
    for bad in (float("nan"), float("inf"), -float("inf"), 1e39, "0.3", None, True):
        with pytest.raises(ValueError):
            rs.check_threshold(bad)
    sel = IDSelectorRange(0, 10)
    assert unpack_params(None, ivf=True) == (None, None)
    assert unpack_params(SearchParameters(sel=sel), ivf=False) == (sel, None)
    assert unpack_params(SearchParametersIVF(sel=sel, nprobe=7), ivf=True) == (sel, 7)
    with pytest.raises(ValueError):
        unpack_params(SearchParametersIVF(nprobe=7), ivf=False)
    with pytest.raises(ValueError):
        unpack_params({"sel": sel}, ivf=True)
    for name in ("FlatIPIndex", "IVFFlatIPIndex", "IVFSQIPIndex"):
        assert name in rs.UNSUPPORTED and name in rs.NO_SHARDED


def test_refusals_need_no_device():
    from wise_amd.index.flat_ip import FlatIPIndex
    from wise_amd.index.ivf_pq import IVFPQIPIndex
    from wise_amd.index.sharded import ShardedFlatIPIndex
    pq = IVFPQIPIndex(32, 4, 8, device="cpu")
    with pytest.raises(NotImplementedError, match="IVFSQIPIndex"):
        pq.range_search(np.zeros((1, 32), np.float32), 0.5)
    with pytest.raises(NotImplementedError, match="IVFFlatIPIndex"):
        pq.range_search_device(None, 0.5)
    sh = ShardedFlatIPIndex(FlatIPIndex(16, device="cpu"))
    with pytest.raises(NotImplementedError, match="sharded"):
        sh.range_search(np.zeros((1, 16), np.float32), 0.5)
    from wise_amd.index.feature_search_index import FeatureSearchIndex
    assert callable(FeatureSearchIndex.search_range)

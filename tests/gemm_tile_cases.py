"""The case table of tests/test_gpu_gemm_tiles.py: which (tile variant, epilogue mode) kernels of the bf16 GEMM family
(csrc/gemm_bf16.hip, csrc/gemm_w4.h) the suite launches directly, at which shapes, and which pairs the library refuses.
Plain Python, no GPU and no torch: tests/test_gemm_tile_cases_cpu.py holds this table against tests/golden/gemm_plan.txt,
so a tower shape that lands on a kernel missing here fails without a GPU.

Plain GEMM (wise_debug_set_gemm_variant + wise_debug_gemm_rows): PLAIN_CASES, shapes from plain_shapes / persistent_shapes.
Fold forms (wise_gemm_fold_bf16 / wise_gemm_fold_resid; no force knob): FOLD_CASES, shapes searched through fold_plan
(fold_shapes) for the compute units of the device."""
import math
import re

# epilogue modes (csrc/gemm_shared.h)
BF16, QUICKGELU, GELU, RESID, F32, GELU_TANH, RELU = 0, 1, 2, 3, 4, 5, 6
MODES = (BF16, QUICKGELU, GELU, RESID, F32, GELU_TANH, RELU)
BF16_MODES = (BF16, QUICKGELU, GELU, GELU_TANH, RELU)

# variant id -> (tile rows, tile columns): the table at the top of csrc/gemm_bf16.hip
TILE = {0: (128, 128), 1: (128, 128), 2: (128, 128), 5: (256, 192), 40: (256, 256), 42: (320, 256), 44: (320, 128),
        60: (256, 256), 61: (160, 256), 62: (320, 256), 63: (320, 192), 64: (160, 256), 65: (224, 192), 66: (256, 192),
        67: (128, 192), 68: (128, 256), 69: (128, 192), 70: (128, 128)}
VARIANTS = tuple(TILE)
W4 = tuple(range(60, 71))               # the one-wave-per-SIMD kernel of gemm_w4.h
BF16_ONLY = (62, 63, 64)                # no fp32 epilogue (a 320-row tile's spills; the persistent form packs to bf16)
PERSISTENT = 64
# wise_debug_set_gemm_variant(0) means "the plan's own choice", not variant 0 (at K >= 512 a few tiles plan the 64-deep
# ring): variant 0 is forced through an id nobody uses, which resolve_variant sends to its default, the 128 x 128 kernel
FORCE_ID = {0: 3}


def resolves(v, M, N, K, mode):
    """The variant a forced id v != 0 launches on this shape: resolve_variant of csrc/gemm_bf16.hip restated (the rules only: tile
    multiples, bf16-only for 62 / 63 / 64, K >= 192 for 60 - 70, K >= 512 for 64, K % 64 for all but 1 / 40 / 42)."""
    if v in W4:
        rows, cols = TILE[v]
        ok = M % rows == 0 and N % cols == 0 and K % 64 == 0 and K >= (512 if v == PERSISTENT else 192)
        if v in BF16_ONLY and mode not in BF16_MODES:
            ok = False
        return v if ok else 0
    if K % 64 != 0 and v not in (40, 42):
        v = 1
    elif N % 128 != 0 and v != 1:
        v = 0
    if v in (1, 2):
        return v
    if v in (5, 40, 42, 44):
        rows, cols = TILE[v]
        return v if M % rows == 0 and N % cols == 0 else 0
    return 0


# (variant, mode) pairs the resolver refuses on every shape: they fall back to variant 0 and are not run
REFUSED = tuple((v, m) for v in BF16_ONLY for m in (RESID, F32))
# (variant, K) the resolver refuses on every shape: 320 x 128 ping-pong tiles take 32-deep K-tiles themselves, but
# resolve_variant sends every K % 64 != 0 that is not 40 / 42 to the 32-deep ring (variant 1)
REFUSED_K = ((44, 96), (44, 160))
PLAIN_CASES = tuple((v, m) for v in VARIANTS for m in MODES if (v, m) not in REFUSED)

_K = {0: (64, 192, 256, 320, 1024), 1: (32, 96, 160), 2: (512, 576), 5: (64, 192, 320, 1024),
      40: (96, 160, 192, 256, 320, 1024), 42: (96, 160, 192, 256, 320, 1024), 44: (192, 256, 320, 1024)}
_K_W4 = (192, 256, 320, 1024)           # 3, 4, 5 and 16 K-steps
N_EDGE = (36, 96, 288)                  # variants 0 and 1: N that is no multiple of the tile


def grids(v):
    """(tiles_m, tiles_n) of the three tile grids of variant v: one tile, then 3 x 2 and 5 x 3 — a tile count that is no
    multiple of 8 (the XCD remainder of tile_coords), tiles_m != tiles_n, tiles_m no multiple of the group size 4.
    The entry points take M % 128 == 0 only, so tiles of 160, 224 and 320 rows come in units of 4, 4 and 2 row tiles: there
    tiles_m is 1, 3, 5 units (for 160 and 224 rows a multiple of 4, which no shape can avoid).  Variant 5 (256 x 192) takes
    N % 128 == 0 only (resolve_variant sends every other N to variant 0): its column tiles come in pairs."""
    rows = TILE[v][0]
    unit = math.lcm(rows, 128) // rows
    out = []
    for a, b in ((1, 1), (3, 2), (5, 3)):
        tm, tn = a * unit, b * (2 if v == 5 else 1)
        while a > 1 and (tm * tn) % 8 == 0:
            tn += 1
        out.append((tm, tn))
    return out


def plain_shapes(v):
    """(M, N, K) of variant v (not the persistent form): every grid x every K-step count, then the N edge"""
    assert v != PERSISTENT
    rows, cols = TILE[v]
    ks = _K.get(v, _K_W4)
    out = [(tm * rows, tn * cols, K) for tm, tn in grids(v) for K in ks]
    if v in (0, 1):
        out += [(384, N, K) for N in N_EDGE for K in ks[:2]] + [(128, N, ks[-1]) for N in N_EDGE]
    return out


def _factor(count):
    """count tiles of 160 x 256 as tiles_m x tiles_n with tiles_m a multiple of 4 (M % 128 == 0), as square as it goes"""
    assert count % 4 == 0
    best = None
    for a in range(1, count // 4 + 1):
        if (count // 4) % a == 0:
            tm, tn = 4 * a, count // (4 * a)
            if best is None or abs(tm - tn) < abs(best[0] - best[1]):
                best = (tm, tn)
    return best


def persistent_shapes(cus):
    """The persistent form (variant 64) on a device of `cus` compute units: (M, N, K, modes).  K = 512 and 576 are 8 and 9
    K-steps (the shortest its drain allows, and one more).  Tile counts: 12 (fewer than the CUs: every workgroup one
    tile), the first multiple of 4 above cus (some workgroups walk two tiles) and above 2 cus (some walk three).
    M % 128 == 0 and 160-row tiles make tiles_m a multiple of 4 whatever the shape, so neither 6 tiles nor an odd
    tiles_m exists for this entry point."""
    out = []
    for count, modes in ((12, BF16_MODES), ((cus // 4 + 1) * 4, (BF16, QUICKGELU)), ((2 * cus // 4 + 1) * 4, (BF16, GELU))):
        tm, tn = _factor(count)
        for K in (512, 576):
            out.append((tm * 160, tn * 256, K, modes))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Fold forms: (variant, mode, producer) rows.  Consumers: wise_gemm_fold_bf16 in modes 0, 1, 2, 5.  Producers:
# wise_gemm_fold_resid, mode 3 = the accumulating form, mode 4 = the form that starts a stream (group32 bit 1).
# ---------------------------------------------------------------------------------------------------------------------
FOLD_CONSUMER_MODES = (BF16, QUICKGELU, GELU, GELU_TANH)
FOLD_CASES = (tuple((v, m, 0) for v in (60, 61, 64, 66, 67, 68, 69, 70) for m in FOLD_CONSUMER_MODES)
              + tuple((v, RESID, 1) for v in (61, 66, 67, 68, 69, 70))
              + tuple((v, F32, 1) for v in (66, 67, 68, 69, 70)))

_FOLD_N = (128, 192, 256, 384, 512, 576, 768, 1024, 1152, 1536, 2048, 2304, 3072, 4096)
_FOLD_K = (192, 256, 320, 512, 576, 640, 832, 1024)
_FOLD_M_MAX = 32768


def fold_shape_ok(M, N, K, producer, wide96):
    """gemm_fold_shape_ok and the producer's width rule of csrc/gemm_bf16.hip"""
    return (M > 0 and M % 128 == 0 and (N % 128 == 0 or N % 192 == 0) and K % 64 == 0 and K >= 192
            and (not producer or wide96 or N % 128 == 0))


def fold_shapes(plan, cus, v, mode, producer, wide96):
    """The smallest shape (fewest multiply-adds) fold_plan sends to variant v, and the same M x N at the other short K
    (192, 256, 320: 3, 4 and 5 K-steps) where it still lands there.  plan(M, N, K, mode, producer, wide96, cus) -> variant.
    [] if the search finds none."""
    best = None
    for K in _FOLD_K:
        for N in _FOLD_N:
            if not fold_shape_ok(128, N, K, producer, wide96):
                continue
            for M in range(128, _FOLD_M_MAX + 1, 128):
                if best is not None and M * N * K >= best[0] * best[1] * best[2]:
                    break
                if plan(M, N, K, mode, producer, wide96, cus) == v:
                    best = (M, N, K)
                    break
    if best is None:
        return []
    M, N, K = best
    return [best] + [(M, N, K2) for K2 in (192, 256, 320) if K2 != K and plan(M, N, K2, mode, producer, wide96, cus) == v]


# ---------------------------------------------------------------------------------------------------------------------
# tests/golden/gemm_plan.txt
# ---------------------------------------------------------------------------------------------------------------------
def parse_plan_table(text):
    """-> (gemm rows as {(variant, mode)}, fold rows as {(variant, mode, producer)}), each with one label that names it"""
    gemm, fold = {}, {}
    for line in text.splitlines():
        kind = line[:4]
        if kind not in ("gemm", "fold"):
            continue
        left, right = line.split("->")
        mode = int(re.search(r"\bmode=(\d+)", left).group(1))
        variants = [int(x) for x in re.findall(r"\bv=(\d+)", right)]
        assert variants, line
        if kind == "gemm":
            for v in variants:
                gemm.setdefault((v, mode), line)
        else:
            producer = int(re.search(r"\bproducer=(\d+)", left).group(1))
            fold.setdefault((variants[0], mode, producer), line)
    return gemm, fold

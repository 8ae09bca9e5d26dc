// bf16 MFMA GEMM with fused epilogues for the ViT / HTSAT blocks (gfx950).
//
//   C[M,N] = epilogue( A[M,K] @ Wt[N,K]^T + bias[N] )      A, Wt bf16 row-major, fp32 accumulate
//
// Stands behind the four nn.Linear calls per transformer block that open_clip's
// VisionTransformer.forward issues from src/feature/mlfoundation_openclip.py:99.
// Roofline: MFMA-bound (2*M*N*K flop).
//
// Structure: 128x128x64 block tile, 4 waves (2x2), each wave a 64x64 sub-tile = 4x4 MFMA
// 16x16x32 accumulators.  Both operands go HBM/L2 -> LDS with 16-byte LDS-DMA
// (global_load_lds_dwordx4), double-buffered, one barrier per K-step.  The LDS image is
// lane-linear (a DMA's destination is base + lane*16) and XOR-swizzled through the per-lane SOURCE
// address: 16-byte chunk c of row r is stored at chunk c ^ (r & 7), which makes the ds_read_b128
// fragment reads conflict-free.  The product is computed transposed (weights as the MFMA A
// operand, activations as B) so that each lane ends up holding 4 consecutive output columns of one
// row: 8-byte bf16 / 16-byte fp32 epilogue accesses, and the bias is one float4 per lane.
#include <utility>
#include <vector>

#include "common.h"
#include "transformer.h"
#include "ln_row.h"
#include "gemm_shared.h"
#include "gemm_w4.h"

namespace wise {

// ---------------------------------------------------------------------------------------------------------------------
// The tile plan: every tile decision of the family, in host functions that launch nothing.  The entry points further
// down (gemm_bf16, gemm_bf16_rows, gemm_resid_ln_rows, gemm_fold_*, conv3x3_bf16) ask the plan, then launch what it says;
// tests/test_gemm_plan_cpu.py pins it shape by shape through wise_debug_gemm_plan (debug library).
// Variant ids:  0 128x128, two blocks per CU             1 128x128 ring of 32-deep K-tiles (K % 64 != 0)
//               2 128x128 ring of 64-deep K-tiles, one block per CU (skinny problems)      5 256x192
//              40 / 42 / 44 ping-pong 256x256 / 320x256 / 320x128 (one block per CU)
//              60 .. 70 the one-wave-per-SIMD kernel of gemm_w4.h: 60 256x256, 61 160x256, 62 320x256, 63 320x192,
//                       64 160x256 persistent, 65 224x192, 66 256x192, 67 128x192, 68 128x256, 69 128x192 and
//                       70 128x128 at two workgroups per CU
// ---------------------------------------------------------------------------------------------------------------------
struct GemmPlan {
    int splitk = 0;         // K slices of the split-K pair (rows 0..127 through scratch); 0 = not a split-K case
    int n = 1;              // launches of the tiled path: 1, or 2 when M is split between two tiles
    int v[2] = {0, 0};      // variant of each launch, after every shape fallback
    int rows[2] = {0, 0};   // rows of each launch, the second starting where the first ends
};

enum ConvTile { CONV_128x64 = 0, CONV_128x128 = 1, CONV_256x64 = 2, CONV_PP256 = 3 };

// What variant v launches on this shape: a shape it cannot tile falls back to 0 (K % 64 != 0: to 1, the 32-deep ring;
// the ping-pong kernels take 32-deep K-tiles themselves; an N that is no multiple of 128 only to the 128x128 kernels).
static int resolve_variant(int v, int M, int N, int K, int mode) {
    if (v >= 60 && v <= 70) {
        bool ok = false;
        switch (v) {
            case 60: ok = w4_shape_ok(M, N, K, 8); break;
            case 61: ok = w4_shape_ok(M, N, K, 5); break;
            case 62: ok = bf16_out(mode) && w4_shape_ok(M, N, K, 10); break;   // (the fp32 epilogues of a 320-row tile spill)
            case 63: ok = bf16_out(mode) && w4_shape_ok(M, N, K, 10, 6); break;
            case 64: ok = bf16_out(mode) && w4p_shape_ok(M, N, K); break;
            case 65: ok = w4_shape_ok(M, N, K, 7, 6); break;
            case 66: ok = w4_shape_ok(M, N, K, 8, 6); break;
            case 67: case 69: ok = w4_shape_ok(M, N, K, 4, 6); break;
            case 68: ok = w4_shape_ok(M, N, K, 4, 8); break;
            case 70: ok = w4_shape_ok(M, N, K, 4, 4); break;
        }
        return ok ? v : 0;
    }
    if (K % 64 != 0 && v != 40 && v != 42) v = 1;
    else if (N % 128 != 0 && v != 1) v = 0;   // N edge is handled by the 128x128 kernels only
    switch (v) {
        case 1: case 2: return v;
        case 5: return M % 256 == 0 && N % 192 == 0 ? 5 : 0;
        case 40: return M % 256 == 0 && N % 256 == 0 ? 40 : 0;
        case 42: return M % 320 == 0 && N % 256 == 0 ? 42 : 0;
        case 44: return M % 320 == 0 && N % 128 == 0 ? 44 : 0;
        default: return 0;
    }
}

// shape heuristic among the two-blocks-per-CU kernels (measured with tools/gemm_bench.py on MI355X)
static int auto_variant(int M, int N, int K) {
    if (K % 64 != 0) return 1;  // K multiple of 32 only (HTSAT C=96): the BK=32 ring kernel
    // Skinny problems (a text query: 77 rows against [N, K] weights; the heads of the towers): fewer blocks than CUs, each
    // streaming its own slab of the weights from HBM over a long K — latency-bound with one K-tile in flight (12800x...
    // shapes never come here).  The ring kernel keeps four 64-deep K-tiles in flight per block: 256x1024x4096 57 -> 19 us.
    if ((long long)(M / 128) * ((N + 127) / 128) <= 128 && K >= 512) return 2;
    // when a 256x192 tiling fits the chip in ONE well-filled round it beats 128x128 (fewer staged bytes, no
    // second-round tail); otherwise the 128x128 tile at two blocks per CU wins because its epilogue overlaps
    // the other block's main loop
    const long long t5 = (long long)(M / 256) * (N / 192);
    if (M % 256 == 0 && N % 192 == 0 && t5 <= 256 && t5 >= 160) return 5;
    return 0;
}

// The one-wave-per-SIMD kernel (gemm_w4.h) takes every problem it can tile into at least ~3/4 of a round of the 256 CUs.
// Among its tiles the model is rounds x (prologue + K-steps x cycles per step + epilogue) with the cycles its in-kernel
// stamps show on MI355X (tools/gemm_lab.hip; the loops run at 76-79 % of the MFMA rate: 160 x 256 ~1700 cycles per
// 64-deep step, 256 x 256 ~2560, 320 x 192 ~2430, 320 x 256 ~3250; prologue ~3200); the epilogue is bound by the HBM
// traffic of the C tile, i.e. proportional to the tile's area whatever its shape, so it only enters through the
// rounds.  Returns the variant id (60 .. 70) or 0.  cus: the compute units of the device (the persistent form's grid).
static int w4_variant(int M, int N, int K, int mode, int cus) {
    // (K >= 192: three 64-deep K-steps.  Short K used to stay with the two-blocks-per-CU kernels; on the HTSAT shapes —
    // K = 192 / 384 at 131072 / 32768 rows — these tiles measured 5-25 % faster than those: tools/gemm_lab.hip htsat)
    if (K < 192) return 0;
    // Short K (HTSAT's stages: K = 192 / 384, and K = 768 on its 8192-row stage): a tile is a handful of K-steps between a
    // prologue and an epilogue that one workgroup per CU cannot overlap with anything.  Two workgroups of 128 x 192 (or
    // 128 x 128) per CU can: measured 7-22 % faster than the best single tile on the bf16-output shapes and 3-7 % on the
    // residual ones at K <= 384 (profiles/r03_gemm_lab_htsat_two_per_cu.txt); at K >= 768 with many rows the small tiles
    // are LDS-bound and lose to the large ones (ViT-B/32: same file, vit section), so the rule stops there.
    // (K = 512, the CLIP text tower at 256 queries x 77 tokens: QKV 37.3 -> 35.0 us, out-projection 26.4 -> 21.9, fc1
    // 62.9 -> 49.5 — `tools/gemm_lab text`.)
    if ((K <= 512 || (K <= 768 && M <= 8192 && bf16_out(mode))) && !(bf16_out(mode) && w4p_shape_ok(M, N, K))) {
        if (w4_shape_ok(M, N, K, 4, 6) && (long long)(M / 128) * (N / 192) >= 512) return 69;
        if (w4_shape_ok(M, N, K, 4, 4) && (long long)(M / 128) * (N / 128) >= 512) return 70;
    }
    // (Measured and not taken: the same two-per-CU tiles on the output projections of the wide towers — N = K = 1024, fp32
    // residual: 219 -> 194 us alone on ViT-L/14's shape, but no gain in the tower's step with two batches in flight.)
    struct Cand { int id, mi, nj; double step; bool bf16_only; };
    static const Cand cands[] = {{60, 8, 8, 2560.0, false}, {61, 5, 8, 1700.0, false}, {62, 10, 8, 3250.0, true},
                                 {63, 10, 6, 2430.0, true}, {65, 7, 6, 1720.0, false}, {66, 8, 6, 1950.0, false},
                                 {67, 4, 6, 1100.0, false}, {68, 4, 8, 1360.0, false}};
    double best = 0.0;
    int v = 0;
    // The model ranks w4 tiles against each other; it knows nothing of the two-blocks-per-CU kernels.  So the tiles added
    // for HTSAT (66 .. 68) compete only where the choice is inside the family already — one of the older tiles divides the
    // shape — or K < 512, where they were measured against those kernels.  (ViT-L/14 and H/14, M = 129 x 128 and 65 x 128
    // rows with K >= 1024, fit only the new tiles and lose 5 % on them: they stay where they were.)
    // (... or the row count is a multiple of 4096 — HTSAT's token counts — where the new tiles were measured against those
    // kernels on every shape: its stage-3 fc2, 32768 x 384 x 1536, has no older tile that divides N = 384: 58 -> 47 us)
    bool family = K < 512 || M % 4096 == 0;
    for (const Cand& c : cands)
        if (c.id <= 65 && !(c.bf16_only && !bf16_out(mode)) && w4_shape_ok(M, N, K, c.mi, c.nj)) family = true;
    for (const Cand& c : cands) {
        if (c.id > 65 && !family) continue;
        if (c.bf16_only && !bf16_out(mode)) continue;
        if (!w4_shape_ok(M, N, K, c.mi, c.nj)) continue;
        const long long tiles = (long long)(M / (32 * c.mi)) * (N / (32 * c.nj));
        if (tiles < 192) continue;
        const long long rounds = (tiles + 255) / 256;
        const double epilogue = 10500.0 * (c.mi * c.nj / 64.0) * (bf16_out(mode) ? 1.0 : 2.0);
        const double act = (mode == EPI_QUICKGELU || mode == EPI_GELU || mode == EPI_GELU_TANH) ? 5000.0 * (c.mi * c.nj / 40.0) : 0.0;
        // operands beyond what the caches hold (> 64 MB): every CU streams its K-steps from the memory side, and a step
        // cannot be shorter than its bytes at ~28 B per clock and CU (measured: 128 x 256 tiles 1360 -> 1640 cycles per
        // step on ViT-L/14's fc2, 160 x 256 1700 -> 1950 on ViT-B/32's; 256 x 256, fewer bytes per flop, unchanged)
        const bool streams = ((double)M + (double)N) * (double)K * 2.0 > 64.0e6;
        const double step_bytes = (32.0 * c.mi + 32.0 * c.nj) * 128.0;
        const double step = streams && step_bytes / 28.0 > c.step ? step_bytes / 28.0 : c.step;
        const double cost = (double)rounds * (3200.0 + (K / 64) * step + epilogue + act);
        if (v == 0 || cost < best) { best = cost; v = c.id; }
    }
    // the persistent form: no prologue between tiles, the C tile leaves under the next tile's loop; what stays exposed per
    // tile is the packing of the accumulators (~1.9k cycles, ~6.2k with a sigmoid-shaped activation) and ~1.7k of drain
    if (bf16_out(mode) && w4p_shape_ok(M, N, K)) {
        const long long tiles = (long long)(M / 160) * (N / 256);
        if (tiles >= cus) {
            const long long rounds = (tiles + cus - 1) / cus;
            const double pack = (mode == EPI_QUICKGELU || mode == EPI_GELU || mode == EPI_GELU_TANH) ? 6200.0 : 1900.0;
            const bool streams = ((double)M + (double)N) * (double)K * 2.0 > 64.0e6;
            const double cost = 3200.0 + (double)rounds * ((K / 64) * (streams ? 1902.0 : 1660.0) + 1700.0 + pack) + 5000.0;
            if (v == 0 || cost < best) { best = cost; v = 64; }
        }
    }
    return v;
}

// a GEMM whose split-K partials would not fit the scratch is not split
constexpr size_t SPLITK_SCRATCH_CAP = (size_t)24 << 20;

// slices of K for a skinny problem (rows 0..m_valid-1 <= 128 of A carry data); 0: not a split-K case
static int splitk_slices(int M, int m_valid, int N, int K) {
    if (m_valid < 1 || m_valid > 128 || M < 128 || K < 512 || K % 128 != 0 || N % 128 != 0 || N < 128) return 0;
    const int slabs = N / 128;
    int S = 1;
    for (int c : {2, 4, 8, 16, 32}) {     // slices: enough blocks for the chip, at least two K-tiles per slice
        if (K % (c * 64) != 0 || K / c < 128) break;
        S = c;
        if (slabs * c >= 160) break;
    }
    if (S < 2 || (size_t)S * 128 * N * sizeof(float) > SPLITK_SCRATCH_CAP) return 0;
    return S;
}

// The plan of gemm_bf16 (m_valid = 0) and gemm_bf16_rows.  m_valid: the rows of A that carry data (the rest of the M rows
// are padding nobody reads); overlapped: the calling thread runs another stream's kernels beside this one
// (gemm_set_overlapped); cus: compute units of the device; force (debug library): a variant id for A/B runs, which goes
// through the same shape fallbacks and never splits K.
static GemmPlan gemm_plan(int M, int N, int K, int mode, int m_valid, bool overlapped, int cus, int force = 0) {
    GemmPlan p;
    p.rows[0] = M;
    if (force) {
        p.v[0] = resolve_variant(force, M, N, K, mode);
        return p;
    }
    p.splitk = splitk_slices(M, m_valid, N, K);
    auto one = [&](int v) {
        p.v[0] = resolve_variant(v, M, N, K, mode);
        return p;
    };
    if (const int vw = w4_variant(M, N, K, mode, cus)) return one(vw);
    // Two whole batches in flight on two streams (VitEngine.forward_pipelined brackets its calls with wise_overlap_hint):
    // measured in one process (ViT-B/32 bs=256): hint ignored 3.28 ms per step; the lone-stream heuristic minus the
    // 320-row tilings (what follows below) 3.16; 128x128 everywhere 3.20.
    // Tile quantisation decides between the ping-pong tilings: 6400 x 3072 is 300 tiles of 256x256 (two rounds
    // at 59 %) but 240 tiles of 320x256 (one round at 94 %); measured 694 -> 799 TFLOP/s on that shape.
    // (not when the caller overlaps two streams: a 144-KiB one-block-per-CU kernel leaves the other stream's
    // kernels nowhere to run, measured 3.54 -> 3.74 ms per ViT-B/32 step)
    if (!overlapped && M % 320 == 0 && N % 256 == 0) {
        const long long t320 = (long long)(M / 320) * (N / 256), t256 = (long long)(M / 256) * (N / 256);
        const double eff320 = (double)t320 / (double)(((t320 + 255) / 256) * 256);
        const double eff256 = (M % 256 == 0) ? (double)t256 / (double)(((t256 + 255) / 256) * 256) : 0.0;
        if (t320 >= 200 && eff320 >= 0.90 && eff320 > eff256 + 0.04) return one(42);
    }
    // fp32-output GEMMs with a narrow N (the two residual GEMMs of a ViT-B block, N = 768): 320 x 128 tiles of the
    // ping-pong kernel when they fill the chip's 256 CUs almost exactly (12800 x 768: 240 tiles, against 200 tiles of
    // 256 x 192 with a quarter more work each): 12800 x 768 x 3072 77 -> 70 us, x 768 32.6 -> 30.7 us
    if ((mode == EPI_RESID || mode == EPI_F32) && !overlapped && M % 320 == 0 && N % 128 == 0 && K >= 128) {
        const long long t = (long long)(M / 320) * (N / 128);
        const double eff = (double)t / (double)(((t + 255) / 256) * 256);
        if (t >= 200 && t <= 256 && eff >= 0.90) return one(44);
    }
    // The 256x256 ping-pong kernel (one block per CU) has the fastest main loop but no co-resident block to
    // hide its epilogue or its tail.  Give it the rows whose tiles fill whole rounds of the 256 CUs and hand the
    // remaining rows to the two-blocks-per-CU kernels (same stream, so the two launches are ordered).
    if (M % 256 == 0 && N % 256 == 0) {
        const int tiles_m = M / 256, tiles_n = N / 256;
        const long long t256 = (long long)tiles_m * tiles_n;
        const double eff256 = (double)t256 / (double)(((t256 + 255) / 256) * 256);
        // (K < 512: a tile is 6-12 K-steps and its epilogue — the activation above all — is most of its life; the
        // 128x128 kernel's second block per CU covers it: 131072x768x192 with GELU 120 -> 106 us, 32768x1536x384 79 -> 75)
        if (t256 >= 200 && K >= 512 && (eff256 >= 0.85 || (K >= 2048 && eff256 >= 0.80))) return one(40);
        // (measured: worth it only when the ping-pong part spans several rounds; at 1-2 rounds the second
        // launch's own tail and the lost overlap cost more than the 128x128 kernel's slower main loop)
        // ... or from two rounds when what is left over is small (ViT-L/14 half batch: 129 x 4 tiles = 2 rounds + 4)
        if (t256 >= 2 * 256 && K >= 512) {
            const int rounds = (int)(t256 / 256);
            const int m_pp = (rounds * 256) / tiles_n;  // m-tiles whose tiles fill `rounds` rounds (within one row)
            const bool small_rest = (tiles_m - m_pp) * 8 <= tiles_m;
            if (m_pp >= 1 && m_pp < tiles_m && (long long)m_pp * tiles_n >= 200 && (t256 >= 3 * 256 || small_rest)) {
                const int M1 = m_pp * 256, M2 = M - M1;
                p.n = 2;
                p.v[0] = resolve_variant(40, M1, N, K, mode);
                p.rows[0] = M1;
                p.v[1] = resolve_variant(auto_variant(M2, N, K), M2, N, K, mode);
                p.rows[1] = M2;
                return p;
            }
        }
    }
    return one(auto_variant(M, N, K));
}

// The LayerNorm fold (vit.hip's fold mode, HTSAT): every form is a one-wave-per-SIMD tile.  producer: the residual form
// with statistics (mode EPI_RESID: x += ...; EPI_F32: x = ..., the rows that start a stream); wide96: the statistics are
// kept per 32 columns (FoldArgs.group32).  Returns the variant id, 0 if no tile fits.
static int fold_plan(int M, int N, int K, int mode, bool producer, bool wide96, int cus) {
    // (the 160 x 256 producer has a residual form only: the rows that start a stream take 128 x 256 or 128 x 128)
    auto tile = [&](int v) { return producer && mode == EPI_F32 && v == 61 ? (w4_shape_ok(M, N, K, 4, 8) ? 68 : 70) : v; };
    const int v = w4_variant(M, N, K, mode, cus);
    if (v == 61 || v == 68 || v == 70 || ((v == 60 || v == 64) && !producer)) return tile(v);   // (the 256 x 256 residual form with statistics spills)
    // tiles with 96-column wave parts (256 x 192, 128 x 192, 128 x 192 at two workgroups per CU): any consumer; a producer
    // only where the model's statistics are kept per 32 columns (FoldArgs.group32: MS-CLAP's HTSAT, widths 192 / 384 / 768)
    if ((v == 66 || v == 67 || v == 69) && (!producer || wide96)) return v;
    if (N % 128 != 0) return w4_shape_ok(M, N, K, 4, 6) ? ((long long)(M / 128) * (N / 192) >= 512 ? 69 : 67) : 0;
    if (!producer && w4p_shape_ok(M, N, K) && (long long)(M / 160) * (N / 256) >= cus) return 64;
    if (w4_shape_ok(M, N, K, 5, 8) && (long long)(M / 160) * (N / 256) >= 192) return tile(61);
    if (w4_shape_ok(M, N, K, 4, 8) && (long long)(M / 128) * (N / 256) >= 256) return 68;
    return 70;
}

// rows the tiles of conv3x3_bf16 walk: every cell, or the four members of every pooling window (floor: odd leftovers are
// not computed)
static long long conv_rows(int B, int T, int F, bool pool) { return pool ? 4ll * B * (T / 2) * (F / 2) : (long long)B * T * F; }

// The tile of conv3x3_bf16 (M = conv_rows(...)).
static ConvTile conv_plan(long long M, int Cout) {
    // The ping-pong tile (one block per CU) where its tiles fill the chip in well-used rounds — measured per layer with
    // tools/conv_bench.py (64 clips x 10 s): 1006-1162 against 904-1037 TFLOP/s on blocks 3 and 4 (6 and 3 rounds), 1031-1057
    // against 978-996 on block 6 (184 tiles, one round), but 947-971 against 1049-1088 on block 5 (372 tiles = 1.45 rounds);
    // its 256 x 128 form lost everywhere it was tried (block 2: 539-679 against 681-857) and is not used.
    const long long tpp = ((M + 255) / 256) * (Cout / 256);
    const double eff = tpp > 0 ? (double)tpp / (double)(((tpp + 255) / 256) * 256) : 0.0;
    if (Cout % 256 == 0 && tpp >= 160 && eff >= 0.70 && (tpp <= 256 || eff >= 0.85)) return CONV_PP256;
    if (Cout % 128 == 0) return CONV_128x128;
    // 64-channel steps (block 1 of Cnn14): 256 x 64 tiles, every wave a 64 x 64 sub-tile (tools/conv_bench.py)
    if (M >= 256 * 512) return CONV_256x64;
    return CONV_128x64;
}

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = BM * BK * 2;  // 16 KiB per operand per buffer

__device__ __forceinline__ void glds16(const void* gsrc, void* lds_dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}

// stage one 128x64 bf16 tile (rows row0.., k from k0) into a 16 KiB LDS tile
__device__ __forceinline__ void stage_tile(const bf16_t* __restrict__ G, int ld, int row0, int k0,
                                           unsigned char* lds_tile, int wave, int lane, int row_last) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int r = (t * 4 + wave) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ (r & 7);  // logical chunk held at physical chunk (lane&7)
        const int gr = min(row0 + r, row_last);  // N edge: rows past the matrix re-read the last row (never stored)
        const bf16_t* src = G + (size_t)gr * ld + k0 + c * 8;
        glds16(src, lds_tile + (t * 4 + wave) * 1024);
    }
}

__device__ __forceinline__ bf16x8 lds_frag(const unsigned char* lds_tile, int row, int chunk) {
    return *reinterpret_cast<const bf16x8*>(lds_tile + row * 128 + ((chunk ^ (row & 7)) << 4));
}

// acc[i][j][r] = C[m0 + wm*64 + i*16 + (lane&15)][n0 + wn*64 + j*16 + (lane>>4)*4 + r]
template <int MODE>
__device__ __forceinline__ void epilogue(f32x4 (&acc)[4][4], const float* __restrict__ bias, void* __restrict__ out,
                                         int N, int m0, int n0, int wm, int wn, int lane) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + wn * 64 + j * 16 + (lane >> 4) * 4;
        if (n >= N) continue;  // N edge (N % 4 == 0, so a lane's 4 columns are all in or all out)
        float4 bv = bias ? *reinterpret_cast<const float4*>(bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + wm * 64 + i * 16 + (lane & 15);
            float v0 = acc[i][j][0] + bv.x, v1 = acc[i][j][1] + bv.y, v2 = acc[i][j][2] + bv.z,
                  v3 = acc[i][j][3] + bv.w;
            const size_t off = (size_t)m * N + n;
            if (MODE == EPI_RESID) {
                float4* p = reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + off);
                float4 x = *p;
                x.x += v0; x.y += v1; x.z += v2; x.w += v3;
                *p = x;
            } else if (MODE == EPI_F32) {
                *reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + off) = make_float4(v0, v1, v2, v3);
            } else {
                v0 = act_apply<MODE>(v0); v1 = act_apply<MODE>(v1); v2 = act_apply<MODE>(v2); v3 = act_apply<MODE>(v3);
                uint2 pk;
                pk.x = pack_bf16x2(v0, v1);
                pk.y = pack_bf16x2(v2, v3);
                *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(out) + off) = pk;
            }
        }
    }
}


// bf16-output epilogue through LDS: the MFMA layout gives a lane 4 consecutive columns of one row
// (8-byte pieces, 32-byte row segments: four store instructions per 128-byte line).  Each wave writes its
// 64x64 sub-tile to a private LDS image (144-byte row stride) and reads it back row-major, so that every
// global store instruction writes 8 complete 128-byte row segments with 16 bytes per lane.
// Precondition: all waves of the block have finished reading the staging buffers (block barrier).
template <int MODE>
__device__ __forceinline__ void epilogue_lds(f32x4 (&acc)[4][4], const float* __restrict__ bias,
                                             bf16_t* __restrict__ out, int N, int m0, int n0, int wm, int wn, int lane,
                                             int wave, unsigned char* smem) {
    constexpr int RS = 144;
    unsigned char* my = smem + wave * (64 * RS);
    const int l15 = lane & 15, g = lane >> 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + wn * 64 + j * 16 + g * 4;
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bias && n < N) bv = *reinterpret_cast<const float4*>(bias + n);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v0 = acc[i][j][0] + bv.x, v1 = acc[i][j][1] + bv.y, v2 = acc[i][j][2] + bv.z,
                  v3 = acc[i][j][3] + bv.w;
            v0 = act_apply<MODE>(v0); v1 = act_apply<MODE>(v1); v2 = act_apply<MODE>(v2); v3 = act_apply<MODE>(v3);
            uint2 pk;
            pk.x = pack_bf16x2(v0, v1);
            pk.y = pack_bf16x2(v2, v3);
            *reinterpret_cast<uint2*>(my + (i * 16 + l15) * RS + (j * 16 + g * 4) * 2) = pk;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int chunk = lane & 7;
    const int n = n0 + wn * 64 + chunk * 8;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int row = t * 8 + (lane >> 3);
        const uint4 v = *reinterpret_cast<const uint4*>(my + row * RS + chunk * 16);
        bf16_t* dst = out + (size_t)(m0 + wm * 64 + row) * N + n;
        if (n + 8 <= N)
            *reinterpret_cast<uint4*>(dst) = v;
        else if (n + 4 <= N)
            *reinterpret_cast<uint2*>(dst) = make_uint2(v.x, v.y);
    }
}

// fp32-output epilogue (modes 3 and 4) through LDS, for one 64x64 sub-tile of a wave.  The MFMA layout gives a
// lane 16 bytes of one row and a wave instruction 16 different rows: 64-byte row fragments, half cache lines,
// and for mode 3 a read-modify-write of each of them.  Here the wave parks the sub-tile in a private 16 KiB LDS
// image (256-byte rows, 16-byte chunks XOR-swizzled by row so both directions are conflict-free) and walks it
// row-major: every global access is 4 rows x 256 contiguous bytes.  The residual rows are loaded BEFORE the
// transposition so that their latency hides under it.
// Precondition: the block has finished with the staging buffers (block barrier); `my` is the wave's 16 KiB.
template <int MODE>
__device__ __forceinline__ void epilogue_f32_lds_64x64(const f32x4 (*acc)[4] /*[4][4]*/, const float* __restrict__ bias,
                                                       float* __restrict__ out, int N, int row0, int col0, int lane,
                                                       unsigned char* my) {
    const int l15 = lane & 15, g = lane >> 4;
    const int n = col0 + l15 * 4;           // this lane's 4 columns on the row-major walk
    const bool in = n + 4 <= N;
    float4 res[16];
    if (MODE == EPI_RESID) {
#pragma unroll
        for (int t = 0; t < 16; ++t)
            res[t] = in ? *reinterpret_cast<const float4*>(out + (size_t)(row0 + t * 4 + g) * N + n)
                        : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int nb = col0 + j * 16 + g * 4;
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bias && nb < N) bv = *reinterpret_cast<const float4*>(bias + nb);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = i * 16 + l15;
            const float4 v = make_float4(acc[i][j][0] + bv.x, acc[i][j][1] + bv.y, acc[i][j][2] + bv.z,
                                         acc[i][j][3] + bv.w);
            *reinterpret_cast<float4*>(my + r * 256 + (((j * 4 + g) ^ (r & 15)) << 4)) = v;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int r = t * 4 + g;
        float4 v = *reinterpret_cast<const float4*>(my + r * 256 + ((l15 ^ (r & 15)) << 4));
        if (MODE == EPI_RESID) { v.x += res[t].x; v.y += res[t].y; v.z += res[t].z; v.w += res[t].w; }
        if (in) *reinterpret_cast<float4*>(out + (size_t)(row0 + t * 4 + g) * N + n) = v;
    }
}

// The same for a (RI*16) x (NJ*16) piece of a wave's accumulators (the 8-wave kernels: NJ = 2, 3 or 4 column
// tiles, RI <= 4 row tiles per pass so that the image stays within the wave's share of the dead staging LDS).
// Rows are NJ*64 bytes; chunks are XOR-swizzled when a row has 16 or 8 of them and rotated when it has 12.
template <int MODE, int RI, int NJ>
__device__ __forceinline__ void epilogue_f32_lds_piece(const f32x4 (*acc)[NJ], const float* __restrict__ bias,
                                                       float* __restrict__ out, int N, int row0, int col0, int lane,
                                                       unsigned char* my) {
    constexpr int CH = NJ * 4, RB = NJ * 64, ROWS = RI * 16;
    constexpr int RP = 64 / CH;                       // rows per wave instruction on the row-major walk (4, 5, 8)
    constexpr int IT = (ROWS + RP - 1) / RP;
    const int l15 = lane & 15, g = lane >> 4;
    auto phys = [](int c, int r) { return CH == 12 ? (c + r) % 12 : (c ^ (r & (CH - 1))); };
    const int wr = lane / CH, wc = lane - wr * CH;    // walk: row within the instruction, chunk
    const bool lane_on = wr < RP;
    const int n = col0 + wc * 4;
    const bool in = lane_on && n + 4 <= N;
    float4 res[IT];
    if (MODE == EPI_RESID) {
#pragma unroll
        for (int t = 0; t < IT; ++t) {
            const int r = t * RP + wr;
            res[t] = (in && r < ROWS) ? *reinterpret_cast<const float4*>(out + (size_t)(row0 + r) * N + n)
                                      : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int nb = col0 + j * 16 + g * 4;
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bias && nb < N) bv = *reinterpret_cast<const float4*>(bias + nb);
#pragma unroll
        for (int i = 0; i < RI; ++i) {
            const int r = i * 16 + l15;
            *reinterpret_cast<float4*>(my + r * RB + (phys(j * 4 + g, r) << 4)) =
                make_float4(acc[i][j][0] + bv.x, acc[i][j][1] + bv.y, acc[i][j][2] + bv.z, acc[i][j][3] + bv.w);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int t = 0; t < IT; ++t) {
        const int r = t * RP + wr;
        if (!in || r >= ROWS) continue;
        float4 v = *reinterpret_cast<const float4*>(my + r * RB + (phys(wc, r) << 4));
        if (MODE == EPI_RESID) { v.x += res[t].x; v.y += res[t].y; v.z += res[t].z; v.w += res[t].w; }
        *reinterpret_cast<float4*>(out + (size_t)(row0 + r) * N + n) = v;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a wave's whole MI x NJ accumulator block through epilogue_f32_lds_piece, four row tiles at a time
template <int MODE, int MI, int NJ>
__device__ __forceinline__ void epilogue_f32_lds_wave(const f32x4 (*acc)[NJ], const float* __restrict__ bias,
                                                      float* __restrict__ out, int N, int row0, int col0, int lane,
                                                      unsigned char* my) {
    static_assert(MI == 8 || MI == 10, "row tiles per wave");
    epilogue_f32_lds_piece<MODE, 4, NJ>(acc, bias, out, N, row0, col0, lane, my);
    epilogue_f32_lds_piece<MODE, 4, NJ>(acc + 4, bias, out, N, row0 + 64, col0, lane, my);
    if (MI == 10) epilogue_f32_lds_piece<MODE, 2, NJ>(acc + 8, bias, out, N, row0 + 128, col0, lane, my);
}

template <int MODE>
__global__ __launch_bounds__(256, 2) void gemm_bf16_kernel(const bf16_t* __restrict__ A,
                                                           const bf16_t* __restrict__ Wt,
                                                           const float* __restrict__ bias, int M, int N, int K,
                                                           void* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // smem: [buf][A tile | W tile]
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    // XCD-aware bijective remap: blocks b, b+8, ... share an XCD; give each XCD a contiguous run of tiles
    const int tiles_n = (N + BN - 1) / BN;
    int tm, tn;
    tile_coords(M / BM, tiles_n, 8, &tm, &tn);
    const int m0 = tm * BM, n0 = tn * BN;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = K / BK;
    stage_tile(A, K, m0, 0, smem, wave, lane, M - 1);
    stage_tile(Wt, K, n0, 0, smem + TILE_BYTES, wave, lane, N - 1);

    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        __syncthreads();  // waits vmcnt(0): tile kt landed; everyone done reading buffer cur^1
        if (kt + 1 < nk) {
            unsigned char* nb = smem + (cur ^ 1) * 2 * TILE_BYTES;
            stage_tile(A, K, m0, (kt + 1) * BK, nb, wave, lane, M - 1);
            stage_tile(Wt, K, n0, (kt + 1) * BK, nb + TILE_BYTES, wave, lane, N - 1);
        }
        const unsigned char* At = smem + cur * 2 * TILE_BYTES;
        const unsigned char* Bt = At + TILE_BYTES;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int chunk = s * 4 + (lane >> 4);
            bf16x8 af[4], wf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = lds_frag(At, wm * 64 + i * 16 + (lane & 15), chunk);
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[j] = lds_frag(Bt, wn * 64 + j * 16 + (lane & 15), chunk);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
        }
    }

    if (bf16_out(MODE) && (N & 7) == 0) {
        __syncthreads();  // staging buffers are dead from here on
        epilogue_lds<MODE>(acc, bias, reinterpret_cast<bf16_t*>(out), N, m0, n0, wm, wn, lane, wave, smem);
    } else if (MODE == EPI_RESID || MODE == EPI_F32) {
        __syncthreads();
        epilogue_f32_lds_64x64<MODE>(acc, bias, reinterpret_cast<float*>(out), N, m0 + wm * 64, n0 + wn * 64, lane,
                                     smem + wave * 16384);
    } else {
        epilogue<MODE>(acc, bias, out, N, m0, n0, wm, wn, lane);
    }
}

// (b, t, f) of cell `base + local` of a [B][Tn][Fn] raster, for a wave-uniform `base` (a tile's first cell) and a small
// per-lane `local` <= lmax.  The convolution kernels need the coordinates of every row a lane stages — up to 8 rows, two
// integer divisions each, ~600 VALU instructions per lane in front of a main loop that is nine K-steps long in Cnn14's
// first block.  Here the divisions are done once per wave on the tile's base; a lane adds its offset with a shift and one
// conditional wrap (Fn a power of two and no more than one wrap of t within the tile: every Cnn14 layer but the last);
// other geometries fall back to the per-lane divisions.
struct CellBase {
    int b, t, f, fshift;
    bool fast;
};
__device__ __forceinline__ CellBase cell_base(int base, int Tn, int Fn, int lmax) {
    CellBase cb;
    const int q = base / Fn;
    cb.f = base - q * Fn;
    cb.b = q / Tn;
    cb.t = q - cb.b * Tn;
    cb.fshift = 31 - __clz(Fn);
    cb.fast = (Fn & (Fn - 1)) == 0 && ((cb.f + lmax) >> cb.fshift) < Tn;
    return cb;
}
__device__ __forceinline__ void cell_at(const CellBase& cb, int base, int local, int Tn, int Fn, int* b, int* t, int* f) {
    if (cb.fast) {
        const int x = cb.f + local;
        int y = cb.t + (x >> cb.fshift), bb = cb.b;
        if (y >= Tn) { y -= Tn; ++bb; }
        *f = x & (Fn - 1); *t = y; *b = bb;
    } else {
        const int q = base + local, qf = q / Fn;
        *f = q - qf * Fn;
        *b = qf / Tn;
        *t = qf - *b * Tn;
    }
}

// ------------------------------------------------------------------------------------------------
// 3x3 convolution, stride 1, zero padding 1, over an NHWC bf16 image, as an implicit GEMM on the same 128-row tile:
//   out[p, n] = relu( sum_{tap, c} X[p + dy(tap)*F + dx(tap), c] * Wt[n, tap*Cin + c] + bias[n] ),   p = (b*T + t)*F + f
// (the ConvBlocks of PANNs Cnn14, the audio encoder of MS-CLAP '2022'; BatchNorm is folded into Wt and bias by the
// packer).  There is no im2col buffer: a K-tile is 64 input channels of ONE tap (Cin % 64 == 0), so the A tile of a
// K-step is 128 row segments of 128 bytes whose source addresses differ from the plain GEMM's only by the tap's shift
// — each lane of the LDS-DMA supplies its own source address, and a lane whose neighbour falls outside the image (or
// whose row is past M) points at a 16-byte page of zeros instead.  Per lane the four rows it stages never change, so
// their (t, f) coordinates are divided out once, before the loop.  Everything else — LDS image, swizzle, fragment
// reads, transposed product, epilogue through LDS — is gemm_bf16_kernel's.  NTJ = column tiles per wave: 4 -> 128
// output channels per block, 2 -> 64 (the first block of Cnn14).  Rows are padded: out has ceil128(M) rows.
//
// POOL: the 2x2 average pooling (floor) that follows the second convolution of a ConvBlock, fused.  Because every A
// row is gathered by address anyway, the tile's rows need not be consecutive cells: row wm*64 + i*16 + l of a tile is
// member i (dt = i >> 1, df = i & 1) of the pooling window of output cell q = 32*tile + 16*wm + l.  The four members
// of a window are then the four row tiles acc[0..3][j] of ONE lane — pooling is three adds per value after bias and
// ReLU, no shuffle, no LDS — and the full-resolution tensor is never written (block 1 of Cnn14 at 64 clips x 10 s:
// 787 MB not written and not read back).  M counts window members (4 per output cell); out [B, T/2, F/2, Cout].
// ------------------------------------------------------------------------------------------------
// WMW = waves along the rows: 2 -> 128 x (32 NTJ) tile (waves 2 x 2), 4 -> 256 x (16 NTJ) (waves 4 x 1: a 64-channel
// layer then gives every wave a 64 x 64 sub-tile — 0.5 fragment reads per MFMA instead of 0.75 for the 64 x 32 of the 2 x 2 form).
template <int NTJ, bool POOL, int WMW = 2>
__global__ __launch_bounds__(256, 2) void conv3x3_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ Wt,
                                                         const float* __restrict__ bias,
                                                         const bf16_t* __restrict__ zeros, int T, int F, int Cin, int M,
                                                         int Cout, bf16_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int WNW = 4 / WMW;
    constexpr int BNC = WNW * 16 * NTJ;               // output channels per block
    constexpr int BMR = WMW * 64;                     // rows per block
    constexpr int TAB = BMR * BK * 2;                 // bytes of an A tile
    constexpr int TW = BNC * BK * 2;                  // bytes of a W tile
    constexpr int SBC = TAB + TW;                     // bytes of a stage
    constexpr int RA = BMR / 32, RW = BNC / 32;       // 1-KiB staging rounds per wave: A, W
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int wm = wave / WNW, wn = wave % WNW;
    const int tiles_n = Cout / BNC;
    int tm, tn;
    tile_coords((M + BMR - 1) / BMR, tiles_n, 8, &tm, &tn);
    const int m0 = tm * BMR, n0 = tn * BNC;
    const int K = 9 * Cin, ck = Cin / BK, nk = 9 * ck;

    // the rows this lane stages: position, coordinates, element offset of its 16-byte chunk at tap (0, 0)
    int pt[RA], pf[RA];
    long long poff[RA];
    const int T2 = T >> 1, F2 = F >> 1;
    const int base = POOL ? tm * (BMR / 4) : m0;      // first output cell / first cell of the tile (wave-uniform)
    const CellBase cb = POOL ? cell_base(base, T2, F2, BMR / 4 - 1) : cell_base(base, T, F, BMR - 1);
#pragma unroll
    for (int t = 0; t < RA; ++t) {
        const int r = (t * 4 + wave) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ (r & 7);
        if constexpr (POOL) {
            const int mem = (r >> 4) & 3;
            const int local = (r >> 6) * 16 + (r & 15);                // output cell of this row's window, within the tile
            int b, t2, f2;
            cell_at(cb, base, local, T2, F2, &b, &t2, &f2);
            const int tt = 2 * t2 + (mem >> 1), ff = 2 * f2 + (mem & 1);
            pf[t] = ff;
            pt[t] = (4 * (base + local) < M) ? tt : -4;
            poff[t] = ((long long)(b * T + tt) * F + ff) * Cin + c * 8;
        } else {
            int b, tt, ff;
            cell_at(cb, base, r, T, F, &b, &tt, &ff);
            pf[t] = ff;
            pt[t] = (m0 + r < M) ? tt : -4;           // rows past M: every tap is "outside"
            poff[t] = (long long)(m0 + r) * Cin + c * 8;
        }
    }
    auto stage = [&](int tap, int cc, unsigned char* dst) {
        const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
        const long long shift = (long long)(dy * F + dx) * Cin + cc * BK;
#pragma unroll
        for (int t = 0; t < RA; ++t) {
            const bool in = (unsigned)(pt[t] + dy) < (unsigned)T && (unsigned)(pf[t] + dx) < (unsigned)F;
            glds16(in ? X + poff[t] + shift : zeros, dst + (t * 4 + wave) * 1024);
        }
#pragma unroll
        for (int t = 0; t < RW; ++t) {                // W tile: BNC rows of 128 bytes
            const int r = (t * 4 + wave) * 8 + (lane >> 3);
            const int c = (lane & 7) ^ (r & 7);
            glds16(Wt + (size_t)(n0 + r) * K + (size_t)(tap * ck + cc) * BK + c * 8, dst + TAB + (t * 4 + wave) * 1024);
        }
    };

    f32x4 acc[4][NTJ];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NTJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    int tap = 0, cc = 0;                              // of the K-tile staged NEXT
    stage(0, 0, smem);
    if (++cc == ck) { cc = 0; ++tap; }
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        __syncthreads();  // waits vmcnt(0): tile kt landed; everyone done reading buffer cur^1
        if (kt + 1 < nk) {
            stage(tap, cc, smem + (cur ^ 1) * SBC);
            if (++cc == ck) { cc = 0; ++tap; }
        }
        const unsigned char* At = smem + cur * SBC;
        const unsigned char* Bt = At + TAB;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int chunk = s * 4 + (lane >> 4);
            bf16x8 af[4], wf[NTJ];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = lds_frag(At, wm * 64 + i * 16 + (lane & 15), chunk);
#pragma unroll
            for (int j = 0; j < NTJ; ++j) wf[j] = lds_frag(Bt, wn * (16 * NTJ) + j * 16 + (lane & 15), chunk);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NTJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
        }
    }
    if constexpr (POOL) {
        const int q = tm * (BMR / 4) + wm * 16 + (lane & 15);
#pragma unroll
        for (int j = 0; j < NTJ; ++j) {
            const int n = n0 + wn * (16 * NTJ) + j * 16 + (lane >> 4) * 4;
            const float4 bv = *reinterpret_cast<const float4*>(bias + n);
            float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v0 += fmaxf(acc[i][j][0] + bv.x, 0.f); v1 += fmaxf(acc[i][j][1] + bv.y, 0.f);
                v2 += fmaxf(acc[i][j][2] + bv.z, 0.f); v3 += fmaxf(acc[i][j][3] + bv.w, 0.f);
            }
            uint2 pk;
            pk.x = pack_bf16x2(0.25f * v0, 0.25f * v1);
            pk.y = pack_bf16x2(0.25f * v2, 0.25f * v3);
            if (4 * q < M) *reinterpret_cast<uint2*>(out + (size_t)q * Cout + n) = pk;
        }
    } else if constexpr (NTJ == 4) {
        __syncthreads();  // staging buffers are dead from here on
        epilogue_lds<EPI_RELU>(acc, bias, out, Cout, m0, n0, wm, wn, lane, wave, smem);
    } else {
        // 64 x 32 per wave: a lane's 4 consecutive channels of one position, 8 bytes at a time
#pragma unroll
        for (int j = 0; j < NTJ; ++j) {
            const int n = n0 + wn * (16 * NTJ) + j * 16 + (lane >> 4) * 4;
            const float4 bv = *reinterpret_cast<const float4*>(bias + n);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = m0 + wm * 64 + i * 16 + (lane & 15);
                uint2 pk;
                pk.x = pack_bf16x2(fmaxf(acc[i][j][0] + bv.x, 0.f), fmaxf(acc[i][j][1] + bv.y, 0.f));
                pk.y = pack_bf16x2(fmaxf(acc[i][j][2] + bv.z, 0.f), fmaxf(acc[i][j][3] + bv.w, 0.f));
                *reinterpret_cast<uint2*>(out + (size_t)m * Cout + n) = pk;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Ring-pipelined variant: STAGES LDS stages of one 128 x BK tile pair, loads issued STAGES-1
// K-steps ahead and left in flight across the (raw) barrier behind a COUNTED s_waitcnt vmcnt.
// One barrier per K-step.  BK=64: 128-B rows, chunk swizzle c ^ (r&7).  BK=32: 64-B rows (four
// tile rows per 256-B bank row), chunk swizzle c ^ g((r>>2)&3), g = {0,2,3,1}: conflict-free for the
// ds_read_b128 lane groups of gfx950 (MI355X_MICROARCH.md, LDS table).
// ------------------------------------------------------------------------------------------------
template <int BKT>
__device__ __forceinline__ int swz_chunk(int row, int c) {
    if (BKT == 64) return c ^ (row & 7);
    return c ^ ((0x78 >> (((row >> 2) & 3) * 2)) & 3);
}

template <int BKT>
__device__ __forceinline__ void stage_tile_ring(const bf16_t* __restrict__ G, int ld, int row0, int k0,
                                                unsigned char* lds_tile, int wave, int lane, int row_last) {
    constexpr int RB = BKT * 2;              // row bytes
    constexpr int RPI = 1024 / RB;           // rows per wave-instruction
    constexpr int CPR = RB / 16;             // chunks per row
    constexpr int ROUNDS = 128 * RB / 1024 / 4;
#pragma unroll
    for (int t = 0; t < ROUNDS; ++t) {
        const int r = (t * 4 + wave) * RPI + lane / CPR;
        const int c = swz_chunk<BKT>(r, lane % CPR);  // involution: logical chunk stored at phys (lane % CPR)
        const bf16_t* src = G + (size_t)min(row0 + r, row_last) * ld + k0 + c * 8;
        glds16(src, lds_tile + (t * 4 + wave) * 1024);
    }
}

template <int BKT>
__device__ __forceinline__ bf16x8 lds_frag_ring(const unsigned char* lds_tile, int row, int chunk) {
    return *reinterpret_cast<const bf16x8*>(lds_tile + row * (BKT * 2) + (swz_chunk<BKT>(row, chunk) << 4));
}

template <int MODE, int BKT, int STAGES, int MINB>
__global__ __launch_bounds__(256, MINB) void gemm_ring_kernel(const bf16_t* __restrict__ A,
                                                              const bf16_t* __restrict__ Wt,
                                                              const float* __restrict__ bias, int M, int N, int K,
                                                              void* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int TB = 128 * BKT * 2;        // bytes per operand tile
    constexpr int SB = 2 * TB;               // bytes per stage
    constexpr int GPS = 2 * (TB / 1024 / 4); // glds per thread per K-step
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    const int tiles_n = (N + BN - 1) / BN;
    int tm, tn;
    tile_coords(M / BM, tiles_n, 8, &tm, &tn);
    const int m0 = tm * BM, n0 = tn * BN;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = K / BKT;
#pragma unroll
    for (int s = 0; s < STAGES - 1; ++s) {
        if (s < nk) {
            stage_tile_ring<BKT>(A, K, m0, s * BKT, smem + s * SB, wave, lane, M - 1);
            stage_tile_ring<BKT>(Wt, K, n0, s * BKT, smem + s * SB + TB, wave, lane, N - 1);
        }
    }
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        // tile kt landed once at most the loads of the STAGES-2 younger tiles are outstanding
        if (kt + STAGES - 2 < nk)
            wait_vmcnt<(STAGES - 2) * GPS>();
        else
            wait_vmcnt<0>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        {
            const int nt = kt + STAGES - 1;
            if (nt < nk) {
                int ns = cur + STAGES - 1;
                if (ns >= STAGES) ns -= STAGES;
                stage_tile_ring<BKT>(A, K, m0, nt * BKT, smem + ns * SB, wave, lane, M - 1);
                stage_tile_ring<BKT>(Wt, K, n0, nt * BKT, smem + ns * SB + TB, wave, lane, N - 1);
            }
        }
        const unsigned char* At = smem + cur * SB;
        const unsigned char* Bt = At + TB;
#pragma unroll
        for (int s = 0; s < BKT / 32; ++s) {
            const int chunk = s * 4 + (lane >> 4);
            bf16x8 af[4], wf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = lds_frag_ring<BKT>(At, wm * 64 + i * 16 + (lane & 15), chunk);
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[j] = lds_frag_ring<BKT>(Bt, wn * 64 + j * 16 + (lane & 15), chunk);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
        }
        cur = (cur + 1 == STAGES) ? 0 : cur + 1;
    }
    // the ring (>= 64 KiB for the instantiations in use) is dead after the last fragment read: reuse it for the
    // row-major epilogues (these shapes, K = 96..384 with M in the 10^5s, are bound by their C traffic)
    constexpr bool RING_FITS = STAGES * SB >= 65536;
    if (RING_FITS && bf16_out(MODE) && (N & 7) == 0) {
        __syncthreads();
        epilogue_lds<MODE>(acc, bias, reinterpret_cast<bf16_t*>(out), N, m0, n0, wm, wn, lane, wave, smem);
    } else if (RING_FITS && (MODE == EPI_RESID || MODE == EPI_F32)) {
        __syncthreads();
        epilogue_f32_lds_64x64<MODE>(acc, bias, reinterpret_cast<float*>(out), N, m0 + wm * 64, n0 + wn * 64, lane,
                                     smem + wave * 16384);
    } else {
        epilogue<MODE>(acc, bias, out, N, m0, n0, wm, wn, lane);
    }
}

// ------------------------------------------------------------------------------------------------
// Skinny problems — one text query is 77 rows against [N, K] weights (K up to 4096) — as split-K: the grid is
// (N / 128 column slabs) x (S slices of K), every block runs the ring kernel's loop over ITS slice for rows 0..127 and
// stores the fp32 partial tile; splitk_reduce_kernel adds the S partials in a fixed order (deterministic), then bias and
// the epilogue, for the rows that matter.  256x1024x4096 (XLM-R fc2 of one query): 16 blocks x 64 K-tiles = 57 us as an
// ordinary launch; 128 blocks x 4 K-tiles + the reduction: see tools/text_latency.py.
// ------------------------------------------------------------------------------------------------
template <int STAGES>
__global__ __launch_bounds__(256, 1) void gemm_splitk_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ Wt, int N,
                                                             int K, int k_len, float* __restrict__ part /*[S][128][N]*/) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int BKT = 64;
    constexpr int TB = 128 * BKT * 2, SB = 2 * TB, GPS = 2 * (TB / 1024 / 4);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int n0 = blockIdx.x * BN, k0 = blockIdx.y * k_len;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nk = k_len / BKT;
#pragma unroll
    for (int s = 0; s < STAGES - 1; ++s) {
        if (s < nk) {
            stage_tile_ring<BKT>(A, K, 0, k0 + s * BKT, smem + s * SB, wave, lane, 127);
            stage_tile_ring<BKT>(Wt, K, n0, k0 + s * BKT, smem + s * SB + TB, wave, lane, N - 1);
        }
    }
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + STAGES - 2 < nk)
            wait_vmcnt<(STAGES - 2) * GPS>();
        else
            wait_vmcnt<0>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        {
            const int nt = kt + STAGES - 1;
            if (nt < nk) {
                int ns = cur + STAGES - 1;
                if (ns >= STAGES) ns -= STAGES;
                stage_tile_ring<BKT>(A, K, 0, k0 + nt * BKT, smem + ns * SB, wave, lane, 127);
                stage_tile_ring<BKT>(Wt, K, n0, k0 + nt * BKT, smem + ns * SB + TB, wave, lane, N - 1);
            }
        }
        const unsigned char* At = smem + cur * SB;
        const unsigned char* Bt = At + TB;
#pragma unroll
        for (int s = 0; s < BKT / 32; ++s) {
            const int chunk = s * 4 + (lane >> 4);
            bf16x8 af[4], wf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = lds_frag_ring<BKT>(At, wm * 64 + i * 16 + (lane & 15), chunk);
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[j] = lds_frag_ring<BKT>(Bt, wn * 64 + j * 16 + (lane & 15), chunk);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
        }
        cur = (cur + 1 == STAGES) ? 0 : cur + 1;
    }
    // partial tile, fp32, row-major [128][N] of slice blockIdx.y: lane owns 4 consecutive columns of 16 rows
    float* ps = part + (size_t)blockIdx.y * 128 * N;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + wn * 64 + j * 16 + (lane >> 4) * 4;
        if (n >= N) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = wm * 64 + i * 16 + (lane & 15);
            *reinterpret_cast<float4*>(ps + (size_t)m * N + n) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
        }
    }
}

// out[m, n..n+3] = epi( sum_s part[s][m][n..] + bias ) for m < rows; thread per 4 columns
template <int MODE>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, int S, int rows, int N,
                                                            const float* __restrict__ bias, void* __restrict__ out) {
    const int n4 = N >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * n4) return;
    const int m = idx / n4, c = idx - m * n4;
    float4 v = bias ? reinterpret_cast<const float4*>(bias)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = 0; s < S; ++s) {
        const float4 p = reinterpret_cast<const float4*>(part + ((size_t)s * 128 + m) * N)[c];
        v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
    }
    if (MODE == EPI_RESID) {
        float4* o = reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + (size_t)m * N) + c;
        const float4 r = *o;
        *o = make_float4(r.x + v.x, r.y + v.y, r.z + v.z, r.w + v.w);
    } else if (MODE == EPI_F32) {
        reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + (size_t)m * N)[c] = v;
    } else {
        uint2 pk;
        pk.x = pack_bf16x2(act_apply<MODE>(v.x), act_apply<MODE>(v.y));
        pk.y = pack_bf16x2(act_apply<MODE>(v.z), act_apply<MODE>(v.w));
        reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(out) + (size_t)m * N)[c] = pk;
    }
}

// The reduction of a RESIDUAL split-K GEMM and the LayerNorm that follows it, in one launch (a text query is a chain of
// ~10 dependent launches per layer on 77 rows: every launch removed is ~5 us of latency).  Workgroup per row, thread per
// 4 columns (and per 1024 columns of the row): the S partials of a thread's columns are independent loads, as many
// threads in flight as the plain reduction has — a wave per row, with the S x N/256 loads of a lane in sequence, measured
// SLOWER than the two launches it replaced (XLM-R-large, one query: 2.04 -> 2.78 ms).  x_new = x + (bias + p_0 + p_1 + ...)
// in that fixed order; exact two-pass statistics over the row from ln_row.h's primitives, summed in LnRow's order so that a row
// gets the bits the two launches give it, whichever path its batch size selects: there lane l of ONE wave owns the float4
// columns l, l + 64, l + 128, ... and adds their sums one after the other before the butterfly.  Here thread t owns columns
// t, t + 256, ...: the per-column sums go through LDS in column order, and every wave walks its lane's columns as that one
// wave would (4 NV dependent adds, <= 16) and runs the same butterfly.  Deterministic, call-to-call bit-stable.
// write_norm: post-LN blocks (BERT family) keep the NORMALISED row as the residual.
template <int NV>
__global__ __launch_bounds__(256) void splitk_reduce_ln_kernel(const float* __restrict__ part, int S, int rows, int N,
                                                               const float* __restrict__ bias, float* __restrict__ x,
                                                               const float* __restrict__ lw, const float* __restrict__ lb,
                                                               float eps, bf16_t* __restrict__ y, int write_norm) {
    __shared__ float col[2][NV * 256];     // per float4 column: its sum, then its sum of squared deviations
    const int row = blockIdx.x, t = threadIdx.x, lane = t & 63;
    const int w4 = N >> 2;
    float4* xr = reinterpret_cast<float4*>(x + (size_t)row * N);
    float4 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = i * 256 + t;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < w4) {
            float4 a = bias ? reinterpret_cast<const float4*>(bias)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 r = xr[c];
            const float4* pp = reinterpret_cast<const float4*>(part + (size_t)row * N) + c;
            const size_t ps = (size_t)128 * N / 4;          // float4 stride between slices
            int k = 0;
            for (; k + 4 <= S; k += 4) {                    // four loads in flight, added in slice order
                const float4 p0 = pp[(size_t)k * ps], p1 = pp[(size_t)(k + 1) * ps], p2 = pp[(size_t)(k + 2) * ps],
                             p3 = pp[(size_t)(k + 3) * ps];
                a.x += p0.x; a.y += p0.y; a.z += p0.z; a.w += p0.w;
                a.x += p1.x; a.y += p1.y; a.z += p1.z; a.w += p1.w;
                a.x += p2.x; a.y += p2.y; a.z += p2.z; a.w += p2.w;
                a.x += p3.x; a.y += p3.y; a.z += p3.z; a.w += p3.w;
            }
            for (; k < S; ++k) {
                const float4 p = pp[(size_t)k * ps];
                a.x += p.x; a.y += p.y; a.z += p.z; a.w += p.w;
            }
            v[i] = make_float4(r.x + a.x, r.y + a.y, r.z + a.z, r.w + a.w);
        }
        col[0][c] = ln_sum4(v[i]);
    }
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4 * NV; ++k) s += col[0][k * 64 + lane];
    const float mean = ln_mean(wave_sum(s), N);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = i * 256 + t;
        col[1][c] = c < w4 ? ln_sqdev4(v[i], mean) : 0.f;
    }
    __syncthreads();
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < 4 * NV; ++k) q += col[1][k * 64 + lane];
    const float rstd = ln_rstd(wave_sum(q), N, eps);
    uint2* yr = reinterpret_cast<uint2*>(y + (size_t)row * N);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = i * 256 + t;
        if (c < w4) {
            const float4 n = ln_affine4(v[i], mean, rstd, reinterpret_cast<const float4*>(lw)[c], reinterpret_cast<const float4*>(lb)[c]);
            yr[c] = ln_pack4(n);
            float4 o = v[i];     // (not `write_norm ? n : v[i]`: a choice between two lvalues takes v's address and sends it to scratch)
            if (write_norm) o = n;
            xr[c] = o;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// LayerNorm fused into the GEMM's A operand, for rows short enough that a block holds them whole (K <= 192:
// HTSAT's first two stages, C = 96 / 192, where activations are 0.5M x 96 and every separate pass is a full trip
// through HBM).  C[M,N] = epi( LN(x[M,K]; g, b) @ Wt^T + bias ), bf16 output modes only.
//   1. the block normalises its 128 rows straight from the fp32 residual stream — 8 lanes per row, K/32 float4
//      per lane, two-pass statistics with 3 cross-lane steps — and writes them as bf16 into the LDS image the
//      ring kernels' fragment reads expect (K/32 tiles of 128 x 32, 64-byte rows, chunk swizzle);
//   2. it then walks the column tiles of N itself: the W tile (all of K) arrives by LDS-DMA, K/32 x 16 MFMAs per
//      wave, and the bf16 C tile leaves row-major through the same LDS region the W tile occupied.
// x is read once and the normalised activations never exist in HBM.
// LDS: A image K*256 B + max(W tile K*256 B, 4 x 64 x 144 B epilogue images): 61 KiB at K = 96 (two blocks per CU).
// ------------------------------------------------------------------------------------------------
template <int MODE, int NF /* K / 32 */>
__global__ __launch_bounds__(256, 2) void gemm_ln_kernel(const float* __restrict__ x, const float* __restrict__ lnw,
                                                         const float* __restrict__ lnb, const bf16_t* __restrict__ Wt,
                                                         const float* __restrict__ bias, int M, int N, float eps,
                                                         bf16_t* __restrict__ out) {
    static_assert(bf16_out(MODE), "bf16 output modes only");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int K = NF * 32, TB = 128 * 64;                 // bytes per 128 x 32 bf16 tile
    constexpr int WREG = (NF * TB > 4 * 64 * 144) ? NF * TB : 4 * 64 * 144;
    unsigned char* a_img = smem;                              // [NF][128 rows][64 B]
    unsigned char* w_img = smem + NF * TB;                    // [NF][128 rows][64 B] / epilogue images
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * 128;

    // ---- 1. LayerNorm of rows m0 .. m0+127 into the A image
    {
        const int l8 = threadIdx.x & 7;
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int r = pass * 32 + (threadIdx.x >> 3);
            const float4* xr = reinterpret_cast<const float4*>(x + (size_t)(m0 + r) * K);
            float4 v[NF];
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < NF; ++j) {
                v[j] = xr[j * 8 + l8];
                s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
            }
            s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64);
            const float mean = s / (float)K;
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < NF; ++j) {
                const float a0 = v[j].x - mean, a1 = v[j].y - mean, a2 = v[j].z - mean, a3 = v[j].w - mean;
                q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
            }
            q += __shfl_xor(q, 1, 64); q += __shfl_xor(q, 2, 64); q += __shfl_xor(q, 4, 64);
            const float rstd = rsqrtf(q / (float)K + eps);
#pragma unroll
            for (int j = 0; j < NF; ++j) {
                const float4 g = reinterpret_cast<const float4*>(lnw)[j * 8 + l8];
                const float4 b = reinterpret_cast<const float4*>(lnb)[j * 8 + l8];
                uint2 pk;
                pk.x = pack_bf16x2((v[j].x - mean) * rstd * g.x + b.x, (v[j].y - mean) * rstd * g.y + b.y);
                pk.y = pack_bf16x2((v[j].z - mean) * rstd * g.z + b.z, (v[j].w - mean) * rstd * g.w + b.w);
                // K-tile j, columns 4*l8 .. 4*l8+3: 16-byte chunk l8 >> 1 (swizzled), half l8 & 1
                *reinterpret_cast<uint2*>(a_img + j * TB + r * 64 + (swz_chunk<32>(r, l8 >> 1) << 4) + (l8 & 1) * 8) = pk;
            }
        }
    }
    // ---- 2. column tiles
    const int tiles_n = (N + 127) / 128;
    for (int tn = 0; tn < tiles_n; ++tn) {
        const int n0 = tn * 128;
        __syncthreads();   // A image complete (first trip) / previous epilogue done with w_img
#pragma unroll
        for (int j = 0; j < NF; ++j) stage_tile_ring<32>(Wt, K, n0, j * 32, w_img + j * TB, wave, lane, N - 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        f32x4 acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) acc[i][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            const int chunk = lane >> 4;
            bf16x8 af[4], wf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = lds_frag_ring<32>(a_img + j * TB, wm * 64 + i * 16 + (lane & 15), chunk);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) wf[jj] = lds_frag_ring<32>(w_img + j * TB, wn * 64 + jj * 16 + (lane & 15), chunk);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
                    acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[jj], af[i], acc[i][jj], 0, 0, 0);
        }
        __syncthreads();   // every wave is done reading w_img: it becomes the epilogue's scratch
        epilogue_lds<MODE>(acc, bias, out, N, m0, n0, wm, wn, lane, wave, w_img);
    }
    (void)M; (void)WREG;
}

// ------------------------------------------------------------------------------------------------
// The whole MLP of a C = 96 Swin block in one kernel (HTSAT stage 1, 0.5M tokens): x += fc2(gelu(fc1(LayerNorm(x)))),
// fc1: 96 -> 384, fc2: 384 -> 96, with BOTH weight matrices resident in LDS and nothing else going through it: a persistent workgroup (one per CU,
// 8 waves) stages W1 [384][96] and W2 [96][384] once as MFMA operand images (147 KiB), and every wave takes 32 tokens at a
// time through the whole MLP in registers:
//   x rows -> LayerNorm (4 lanes per token, two-pass) -> bf16 B-operand fragments;
//   per pair of 16-row hidden tiles: h^T = W1 x^T (transposed product: lane = token, registers = hidden rows), + b1, GELU,
//   packed to bf16 — which IS the B operand of the second product y^T += W2 h^T for that 32-deep k-step, because W2's
//   image is stored with its k index permuted the way the first product's accumulators come out;
//   + b2 + x, stored as 16-byte pieces.
// No barrier after the prologue, no LDS write, no staging latency in the loop; what remains is the GELU's VALU work
// (192 values per lane and 32 tokens).  The staged form it replaced re-staged the weight tiles for every 128 rows (600 MB of
// L2 -> LDS traffic per launch) and waited for them four times per block.
// ------------------------------------------------------------------------------------------------
constexpr int MLPR_W1_BYTES = 3 * 384 * 64, MLPR_W2_BYTES = 12 * 96 * 64;

__global__ __launch_bounds__(512, 1) void mlp96r_kernel(float* __restrict__ x, const float* __restrict__ lnw,
                                                        const float* __restrict__ lnb, const bf16_t* __restrict__ W1,
                                                        const float* __restrict__ b1, const bf16_t* __restrict__ W2,
                                                        const float* __restrict__ b2, long long units /*of 32 tokens*/, float eps) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int C = 96, HID = 384;
    unsigned char* w1_img = smem;                                  // [ks 3][384 hidden rows][64 B], 16-byte chunks swizzled
    unsigned char* w2_img = smem + MLPR_W1_BYTES;                  // [hp 12][96 out rows][64 B]: chunk g = hidden (2hp)*16+4g..+3 | (2hp+1)*16+4g..+3
    float* fb = reinterpret_cast<float*>(smem + MLPR_W1_BYTES + MLPR_W2_BYTES);   // b1[384] | b2[96] | ln_w[96] | ln_b[96]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;

    // ---- prologue: the weight images (each 16-byte chunk once)
    for (int c = tid; c < 3 * HID * 4; c += 512) {
        const int ks = c / (HID * 4), rem = c - ks * (HID * 4), row = rem >> 2, ch = rem & 3;
        const uint4 v = *reinterpret_cast<const uint4*>(W1 + (size_t)row * C + ks * 32 + ch * 8);
        *reinterpret_cast<uint4*>(w1_img + ks * (HID * 64) + row * 64 + (swz_chunk<32>(row, ch) << 4)) = v;
    }
    for (int c = tid; c < 12 * C * 4; c += 512) {
        const int hp = c / (C * 4), rem = c - hp * (C * 4), row = rem >> 2, ch = rem & 3;
        const uint2 lo = *reinterpret_cast<const uint2*>(W2 + (size_t)row * HID + (2 * hp) * 16 + ch * 4);
        const uint2 hi = *reinterpret_cast<const uint2*>(W2 + (size_t)row * HID + (2 * hp + 1) * 16 + ch * 4);
        *reinterpret_cast<uint4*>(w2_img + hp * (C * 64) + row * 64 + (swz_chunk<32>(row, ch) << 4)) = make_uint4(lo.x, lo.y, hi.x, hi.y);
    }
    for (int c = tid; c < HID + 3 * C; c += 512)
        fb[c] = c < HID ? b1[c] : (c < HID + C ? b2[c - HID] : (c < HID + 2 * C ? lnw[c - HID - C] : lnb[c - HID - 2 * C]));
    __syncthreads();
    const float* b1s = fb;
    const float* b2s = fb + HID;
    const float* gws = fb + HID + C;
    const float* gbs = fb + HID + 2 * C;

    const long long gw = (long long)blockIdx.x * 8 + wave, nw = (long long)gridDim.x * 8;
    // the rows of the NEXT unit travel while the current one is computed (48 registers)
    float4 xn[2][3][2];
    auto fetch = [&](long long u) {
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const float* xr = x + ((size_t)u * 32 + tt * 16 + l15) * C + g * 8;
#pragma unroll
            for (int ks = 0; ks < 3; ++ks) {
                xn[tt][ks][0] = *reinterpret_cast<const float4*>(xr + ks * 32);
                xn[tt][ks][1] = *reinterpret_cast<const float4*>(xr + ks * 32 + 4);
            }
        }
    };
    if (gw < units) fetch(gw);
    for (long long u = gw; u < units; u += nw) {
        float* xu = x + (size_t)u * 32 * C;
        // ---- LayerNorm -> B-operand fragments af[tt][ks]: lane (token tt*16 + l15, channels ks*32 + g*8 .. +7)
        bf16x8 af[2][3];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            float v[3][8];
            float sm = 0.f;
#pragma unroll
            for (int ks = 0; ks < 3; ++ks) {
                const float4 a = xn[tt][ks][0], bq = xn[tt][ks][1];
                v[ks][0] = a.x; v[ks][1] = a.y; v[ks][2] = a.z; v[ks][3] = a.w;
                v[ks][4] = bq.x; v[ks][5] = bq.y; v[ks][6] = bq.z; v[ks][7] = bq.w;
#pragma unroll
                for (int e = 0; e < 8; ++e) sm += v[ks][e];
            }
            sm += __shfl_xor(sm, 16, 64);
            sm += __shfl_xor(sm, 32, 64);
            const float mean = sm * (1.f / 96.f);
            float sq = 0.f;
#pragma unroll
            for (int ks = 0; ks < 3; ++ks)
#pragma unroll
                for (int e = 0; e < 8; ++e) { v[ks][e] -= mean; sq = fmaf(v[ks][e], v[ks][e], sq); }
            sq += __shfl_xor(sq, 16, 64);
            sq += __shfl_xor(sq, 32, 64);
            const float rstd = rsqrtf(sq * (1.f / 96.f) + eps);
#pragma unroll
            for (int ks = 0; ks < 3; ++ks) {
                const float4 w0 = *reinterpret_cast<const float4*>(gws + ks * 32 + g * 8), w1v = *reinterpret_cast<const float4*>(gws + ks * 32 + g * 8 + 4);
                const float4 c0 = *reinterpret_cast<const float4*>(gbs + ks * 32 + g * 8), c1v = *reinterpret_cast<const float4*>(gbs + ks * 32 + g * 8 + 4);
                const float gw8[8] = {w0.x, w0.y, w0.z, w0.w, w1v.x, w1v.y, w1v.z, w1v.w};
                const float gb8[8] = {c0.x, c0.y, c0.z, c0.w, c1v.x, c1v.y, c1v.z, c1v.w};
                bf16x8 f;
#pragma unroll
                for (int e = 0; e < 8; ++e) f[e] = (__bf16)((v[ks][e] * rstd) * gw8[e] + gb8[e]);
                af[tt][ks] = f;
            }
        }
        if (u + nw < units) fetch(u + nw);
        // ---- the two products, one 32-deep hidden k-step at a time
        f32x4 acc2[6][2];
#pragma unroll
        for (int ct = 0; ct < 6; ++ct)
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) acc2[ct][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int hp = 0; hp < 12; ++hp) {
            bf16x8 hf[2];
            f32x4 a1[2][2];                                    // [hidden tile of the pair][token tile]
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const int hrow = (2 * hp + hh) * 16 + l15;
                const float4 bv = *reinterpret_cast<const float4*>(b1s + (2 * hp + hh) * 16 + g * 4);
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) a1[hh][tt] = f32x4{bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                for (int ks = 0; ks < 3; ++ks) {
                    const bf16x8 wf = *reinterpret_cast<const bf16x8*>(w1_img + ks * (HID * 64) + hrow * 64 + (swz_chunk<32>(hrow, g) << 4));
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt)
                        a1[hh][tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af[tt][ks], a1[hh][tt], 0, 0, 0);
                }
            }
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                bf16x8 f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    f[r] = (__bf16)act_gelu(a1[0][tt][r]);
                    f[4 + r] = (__bf16)act_gelu(a1[1][tt][r]);
                }
                hf[tt] = f;
            }
#pragma unroll
            for (int ct = 0; ct < 6; ++ct) {
                const int orow = ct * 16 + l15;
                const bf16x8 wf = *reinterpret_cast<const bf16x8*>(w2_img + hp * (C * 64) + orow * 64 + (swz_chunk<32>(orow, g) << 4));
#pragma unroll
                for (int tt = 0; tt < 2; ++tt)
                    acc2[ct][tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, hf[tt], acc2[ct][tt], 0, 0, 0);
            }
        }
        // ---- + b2 + residual: lane (token tt*16 + l15): channels ct*16 + g*4 .. +3
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            float* xr = xu + (size_t)(tt * 16 + l15) * C + g * 4;
#pragma unroll
            for (int ct = 0; ct < 6; ++ct) {
                const float4 r = *reinterpret_cast<const float4*>(xr + ct * 16);
                const float4 bb = *reinterpret_cast<const float4*>(b2s + ct * 16 + g * 4);
                *reinterpret_cast<float4*>(xr + ct * 16) = make_float4(r.x + bb.x + acc2[ct][tt][0], r.y + bb.y + acc2[ct][tt][1],
                                                                         r.z + bb.z + acc2[ct][tt][2], r.w + bb.w + acc2[ct][tt][3]);
            }
        }
    }
}

template <int MODE, int NF>
static void launch_gemm_ln(const float* x, const float* lnw, const float* lnb, const bf16_t* Wt, const float* bias,
                           int M, int N, float eps, bf16_t* out, hipStream_t st) {
    auto kern = gemm_ln_kernel<MODE, NF>;
    constexpr size_t TBs = 128 * 64;
    const size_t wreg = (NF * TBs > (size_t)4 * 64 * 144) ? NF * TBs : (size_t)4 * 64 * 144;
    const size_t lds = NF * TBs + wreg;
    static PerDeviceOnce attr_set;
    attr_set([&] {
        raise_lds_limit(reinterpret_cast<const void*>(kern), (int)lds);
    });
    hipLaunchKernelGGL(kern, dim3(M / 128), dim3(256), lds, st, x, lnw, lnb, Wt, bias, M, N, eps, out);
}

template <int MODE, int BKT, int STAGES, int MINB>
static void launch_ring(const bf16_t* A, const bf16_t* Wt, const float* bias, int M, int N, int K, void* out,
                        hipStream_t st) {
    auto kern = gemm_ring_kernel<MODE, BKT, STAGES, MINB>;
    const size_t lds = (size_t)STAGES * 2 * 128 * BKT * 2;
    static PerDeviceOnce attr_set;
    attr_set([&] {
        raise_lds_limit(reinterpret_cast<const void*>(kern), (int)lds);
    });
    const int grid = (M / BM) * ((N + BN - 1) / BN);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, A, Wt, bias, M, N, K, out);
}

template <int MODE>
static void launch_gemm(const bf16_t* A, const bf16_t* Wt, const float* bias, int M, int N, int K, void* out,
                        hipStream_t st) {
    auto kern = gemm_bf16_kernel<MODE>;
    const size_t lds = 4 * TILE_BYTES;  // 64 KiB
    static PerDeviceOnce attr_set;
    attr_set([&] {
        raise_lds_limit(reinterpret_cast<const void*>(kern), (int)lds);
    });
    const int grid = (M / BM) * ((N + BN - 1) / BN);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, A, Wt, bias, M, N, K, out);
}

// ------------------------------------------------------------------------------------------------
// Large-tile kernel: 256 x (64*NT) block tile, 8 waves as 2(M) x 4(N), each wave 128 x (16*NT):
// half the staged bytes per flop of the 128x128 tile (staging, not MFMA, bounds that one: measured
// 13.5 TB/s L2->LDS chip-wide).  Same LDS image, swizzle and transposed-product epilogue.
// ------------------------------------------------------------------------------------------------
template <int MODE, int NT, int MI = 8>
__device__ __forceinline__ void epilogue_big(f32x4 (&acc)[MI][NT], const float* __restrict__ bias,
                                             void* __restrict__ out, int N, int m0, int n0, int wm, int wn, int lane) {
    // epilogue: acc[i][j][r] = C[m0 + wm*128 + i*16 + (lane&15)][n0 + wn*16*NT + j*16 + (lane>>4)*4 + r]
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = n0 + wn * (16 * NT) + j * 16 + (lane >> 4) * 4;
        float4 bv = bias ? *reinterpret_cast<const float4*>(bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int m = m0 + wm * (MI * 16) + i * 16 + (lane & 15);
            float v0 = acc[i][j][0] + bv.x, v1 = acc[i][j][1] + bv.y, v2 = acc[i][j][2] + bv.z,
                  v3 = acc[i][j][3] + bv.w;
            const size_t off = (size_t)m * N + n;
            if (MODE == EPI_RESID) {
                float4* p = reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + off);
                float4 x = *p;
                x.x += v0; x.y += v1; x.z += v2; x.w += v3;
                *p = x;
            } else if (MODE == EPI_F32) {
                *reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + off) = make_float4(v0, v1, v2, v3);
            } else {
                v0 = act_apply<MODE>(v0); v1 = act_apply<MODE>(v1); v2 = act_apply<MODE>(v2); v3 = act_apply<MODE>(v3);
                uint2 pk;
                pk.x = pack_bf16x2(v0, v1);
                pk.y = pack_bf16x2(v2, v3);
                *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(out) + off) = pk;
            }
        }
    }
}

template <int ROWS>
__device__ __forceinline__ void stage_rows8(const bf16_t* __restrict__ G, int ld, int row0, int k0,
                                            unsigned char* lds_tile, int wave, int lane) {
    // ROWS x 64 bf16 tile, 8 waves: wave-instruction u = t*8 + wave covers rows 8u .. 8u+7
#pragma unroll
    for (int t = 0; t < ROWS / 64; ++t) {
        const int u = t * 8 + wave;
        const int r = u * 8 + (lane >> 3);
        const int c = (lane & 7) ^ (r & 7);
        glds16(G + (size_t)(row0 + r) * ld + k0 + c * 8, lds_tile + u * 1024);
    }
}

template <int MODE, int NT>
__global__ __launch_bounds__(512, 2) void gemm_big_kernel(const bf16_t* __restrict__ A,
                                                                    const bf16_t* __restrict__ Wt,
                                                                    const float* __restrict__ bias, int M, int N, int K,
                                                                    void* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int BMB = 256, BNB = 64 * NT;
    constexpr int TA = BMB * 128, TBb = BNB * 128, SB = TA + TBb;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int wm = wave >> 2, wn = wave & 3;

    const int tiles_n = N / BNB;
    int tm, tn;
    tile_coords(M / BMB, tiles_n, 4, &tm, &tn);
    const int m0 = tm * BMB, n0 = tn * BNB;

    f32x4 acc[8][NT];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = K / 64;
    stage_rows8<BMB>(A, K, m0, 0, smem, wave, lane);
    stage_rows8<BNB>(Wt, K, n0, 0, smem + TA, wave, lane);
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        __syncthreads();
        if (kt + 1 < nk) {
            unsigned char* nb = smem + (cur ^ 1) * SB;
            stage_rows8<BMB>(A, K, m0, (kt + 1) * 64, nb, wave, lane);
            stage_rows8<BNB>(Wt, K, n0, (kt + 1) * 64, nb + TA, wave, lane);
        }
        const unsigned char* At = smem + cur * SB;
        const unsigned char* Bt = At + TA;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int chunk = s * 4 + (lane >> 4);
            bf16x8 wf[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) wf[j] = lds_frag(Bt, wn * (16 * NT) + j * 16 + (lane & 15), chunk);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const bf16x8 af = lds_frag(At, wm * 128 + i * 16 + (lane & 15), chunk);
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af, acc[i][j], 0, 0, 0);
            }
        }
    }
    if (MODE == EPI_RESID || MODE == EPI_F32) {
        __syncthreads();  // staging buffers are dead; each wave takes SB*2/8 >= 12 KiB of them
        epilogue_f32_lds_wave<MODE, 8, NT>(acc, bias, reinterpret_cast<float*>(out), N, m0 + wm * 128,
                                           n0 + wn * (16 * NT), lane, smem + wave * (2 * SB / 8));
    } else {
        epilogue_big<MODE, NT>(acc, bias, out, N, m0, n0, wm, wn, lane);
    }
}

template <int MODE, int NT>
static void launch_big(const bf16_t* A, const bf16_t* Wt, const float* bias, int M, int N, int K, void* out,
                       hipStream_t st) {
    auto kern = gemm_big_kernel<MODE, NT>;
    const size_t lds = (size_t)2 * (256 + 64 * NT) * 128;
    static PerDeviceOnce attr_set;
    attr_set([&] {
        raise_lds_limit(reinterpret_cast<const void*>(kern), (int)lds);
    });
    const int grid = (M / 256) * (N / (64 * NT));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, A, Wt, bias, M, N, K, out);
}

// Big tile + ring pipeline: 256 x (64*NT) tile, 8 waves, STAGES stages of BKT-deep tiles, loads kept
// in flight across the raw barrier behind a counted vmcnt (one barrier per K-step).
template <int ROWS, int BKT>
__device__ __forceinline__ void stage_rows8_ring(const bf16_t* __restrict__ G, int ld, int row0, int k0,
                                                 unsigned char* lds_tile, int wave, int lane) {
    constexpr int RB = BKT * 2, RPI = 1024 / RB, CPR = RB / 16;
    constexpr int UNITS = ROWS * RB / 1024;        // 1-KiB wave instructions in the tile
    constexpr int ROUNDS = (UNITS + 7) / 8;        // the last round may be partial (320-row tile: waves 0-3 only)
#pragma unroll
    for (int t = 0; t < ROUNDS; ++t) {
        const int u = t * 8 + wave;
        if (UNITS % 8 != 0 && u >= UNITS) break;
        const int r = u * RPI + lane / CPR;
        const int c = swz_chunk<BKT>(r, lane % CPR);
        glds16(G + (size_t)(row0 + r) * ld + k0 + c * 8, lds_tile + u * 1024);
    }
}

// bf16 epilogue through LDS for the 8-wave 256x256 tile (wave = 128 rows x 64 columns): same idea as
// epilogue_lds, done in two 64-row halves so the eight wave-private images (64 x 144 B) fit 128 KiB.
// Precondition: block barrier after the last fragment read.
template <int MODE, int MI = 8>
__device__ __forceinline__ void epilogue_big_lds(f32x4 (&acc)[MI][4], const float* __restrict__ bias,
                                                 bf16_t* __restrict__ out, int N, int m0, int n0, int wm, int wn,
                                                 int lane, int wave, unsigned char* smem) {
    constexpr int RS = 144, HI = MI / 2, HROWS = HI * 16;  // i-tiles / rows per half (MI = 8: 64, MI = 10: 80)
    unsigned char* my = smem + wave * (HROWS * RS);
    const int l15 = lane & 15, g = lane >> 4;
    const int chunk = lane & 7;
    const int ncol = n0 + wn * 64 + chunk * 8;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wn * 64 + j * 16 + g * 4;
            float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (bias) bv = *reinterpret_cast<const float4*>(bias + n);
#pragma unroll
            for (int ii = 0; ii < HI; ++ii) {
                const int i = half * HI + ii;
                float v0 = acc[i][j][0] + bv.x, v1 = acc[i][j][1] + bv.y, v2 = acc[i][j][2] + bv.z,
                      v3 = acc[i][j][3] + bv.w;
                v0 = act_apply<MODE>(v0); v1 = act_apply<MODE>(v1); v2 = act_apply<MODE>(v2); v3 = act_apply<MODE>(v3);
                uint2 pk;
                pk.x = pack_bf16x2(v0, v1);
                pk.y = pack_bf16x2(v2, v3);
                *reinterpret_cast<uint2*>(my + (ii * 16 + l15) * RS + (j * 16 + g * 4) * 2) = pk;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int t = 0; t < HROWS / 8; ++t) {
            const int row = t * 8 + (lane >> 3);
            const uint4 v = *reinterpret_cast<const uint4*>(my + row * RS + chunk * 16);
            uint4* gdst = reinterpret_cast<uint4*>(out + (size_t)(m0 + wm * (MI * 16) + half * HROWS + row) * N + ncol);
            // non-temporal: the C tile is read by a later kernel, not by this one (ViT-L/14 +1.5 % end to end, ViT-B/32
            // unchanged)
            typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
            __builtin_nontemporal_store(u32x4_t{v.x, v.y, v.z, v.w}, reinterpret_cast<u32x4_t*>(gdst));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// ------------------------------------------------------------------------------------------------
// Ping-pong kernel: 256x256 tile, 8 waves, 4-stage ring of 32-deep K-tiles (128 KiB LDS, one block per
// CU).  Each K-tile is two barrier-separated parts per wave: L = {counted vmcnt, barrier, issue the
// LDS-DMA of tile kt+3, read this tile's 12 fragments} and M = {32 MFMAs on registers only}.  Waves 4-7
// execute ONE extra barrier before the loop (waves 0-3 one after it), so the two waves that share a SIMD
// are always half a step apart: while one issues its MFMA cluster the other is in its L part.
//   RAW: before EVERY barrier a wave waits until its own loads of the tile the OTHER group will read
//        next have landed (at most the two youngest tiles stay in flight);
//   WAR: tile kt+3 overwrites the slot of tile kt-1, whose fragment reads both groups retired
//        (lgkmcnt(0)) before the barrier that precedes the overwrite.
// ------------------------------------------------------------------------------------------------
// WROWS = rows per wave: 128 -> 256x256 tile (waves 2x4, 4 stages of 32 KiB); 80 -> 320x128 tile (waves 4x2, 4 stages
// of 28 KiB) for the narrow fp32-output GEMMs; 160 -> 320x256 tile
// (waves 2x4, 4 stages of 36 KiB) for shapes that fill the chip in whole rounds only with 320-row tiles
// (M = 6400, N = 3072: 240 tiles).  A 320-row A tile is 20 KiB per stage = 2.5 rounds of the 8 waves, so waves
// 0-3 (the early group) issue one LDS-DMA more per K-tile than waves 4-7: the counted vmcnt differs per group.
template <int MODE, int WROWS>
__global__ __launch_bounds__(512, 2) void gemm_pp_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ Wt,
                                                         const float* __restrict__ bias, int M, int N, int K,
                                                         void* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int BKT = 32, NT = 4, MI = WROWS / 16;
    constexpr int BMB = (WROWS == 80) ? 320 : 2 * WROWS;   // 80: 320 x 128, four wave rows
    constexpr int WM_WAVES = BMB / WROWS, WN_WAVES = 8 / WM_WAVES, BNB = WN_WAVES * 64;
    constexpr int STAGES = 4;
    constexpr int TA = BMB * BKT * 2, TBt = BNB * BKT * 2, SB = TA + TBt;
    // LDS-DMA instructions per thread per K-tile: waves 0-3 take the partial last round of a 320-row A tile
    constexpr int GPS_E = (TA / 1024 + 7) / 8 + TBt / 8192, GPS_L = TA / 8192 + TBt / 8192;
    constexpr int INFL_E = (STAGES - 2) * GPS_E, INFL_L = (STAGES - 2) * GPS_L;  // STAGES-2 youngest tiles in flight
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int wm = wave / WN_WAVES, wn = wave % WN_WAVES;
    const bool late = __builtin_amdgcn_readfirstlane(threadIdx.x) >= 256;  // waves 4-7 run half a step behind
    auto wait_inflight = [&]() { if (INFL_E == INFL_L || late) wait_vmcnt<INFL_L>(); else wait_vmcnt<INFL_E>(); };

    const int tiles_n = N / BNB;
    int tm, tn;
    tile_coords(M / BMB, tiles_n, 4, &tm, &tn);
    const int m0 = tm * BMB, n0 = tn * BNB;

    f32x4 acc[MI][NT];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nk = K / BKT;
#pragma unroll
    for (int s = 0; s < STAGES - 1; ++s) {
        if (s < nk) {
            stage_rows8_ring<BMB, BKT>(A, K, m0, s * BKT, smem + s * SB, wave, lane);
            stage_rows8_ring<BNB, BKT>(Wt, K, n0, s * BKT, smem + s * SB + TA, wave, lane);
        }
    }
    if (late) {
        // the early group reads tile 0 right after this barrier: my share of it must have landed
        if (nk >= STAGES - 1) wait_inflight(); else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
    }
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        // ---- L part
        if (kt + STAGES - 2 < nk) wait_inflight(); else wait_vmcnt<0>();   // my share of tile kt has landed
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (kt + STAGES - 1 < nk) {
            int ns = cur + STAGES - 1;
            if (ns >= STAGES) ns -= STAGES;
            stage_rows8_ring<BMB, BKT>(A, K, m0, (kt + STAGES - 1) * BKT, smem + ns * SB, wave, lane);
            stage_rows8_ring<BNB, BKT>(Wt, K, n0, (kt + STAGES - 1) * BKT, smem + ns * SB + TA, wave, lane);
        }
        const unsigned char* At = smem + cur * SB;
        const unsigned char* Bt = At + TA;
        const int chunk = lane >> 4;
        bf16x8 wf[NT], af[MI];
#pragma unroll
        for (int j = 0; j < NT; ++j) wf[j] = lds_frag_ring<BKT>(Bt, wn * 64 + j * 16 + (lane & 15), chunk);
#pragma unroll
        for (int i = 0; i < MI; ++i) af[i] = lds_frag_ring<BKT>(At, wm * WROWS + i * 16 + (lane & 15), chunk);
        // my share of tile kt+1 has landed before the barrier after which the other group may read it
        if (kt + STAGES - 1 < nk) wait_inflight(); else wait_vmcnt<0>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        // ---- M part: registers only
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        cur = (cur + 1 == STAGES) ? 0 : cur + 1;
    }
    if (!late) __builtin_amdgcn_s_barrier();
    constexpr bool BF16OUT = bf16_out(MODE);
    if constexpr (WROWS == 80) {
        if (!BF16OUT) {
            __syncthreads();  // the ring (112 KiB) is dead: 14 KiB of it per wave, pieces of 32 rows x 256 B
            unsigned char* my = smem + wave * 14336;
            float* o = reinterpret_cast<float*>(out);
            epilogue_f32_lds_piece<MODE, 2, NT>(acc, bias, o, N, m0 + wm * WROWS, n0 + wn * 64, lane, my);
            epilogue_f32_lds_piece<MODE, 2, NT>(acc + 2, bias, o, N, m0 + wm * WROWS + 32, n0 + wn * 64, lane, my);
            epilogue_f32_lds_piece<MODE, 1, NT>(acc + 4, bias, o, N, m0 + wm * WROWS + 64, n0 + wn * 64, lane, my);
        } else {
            epilogue_big<MODE, NT, MI>(acc, bias, out, N, m0, n0, wm, wn, lane);
        }
    } else if constexpr (BF16OUT) {
        __syncthreads();  // both groups are past their last fragment read: the ring is dead
        epilogue_big_lds<MODE, MI>(acc, bias, reinterpret_cast<bf16_t*>(out), N, m0, n0, wm, wn, lane, wave, smem);
    } else {
        __syncthreads();  // the ring is dead: 16 KiB (18 KiB) of it per wave
        epilogue_f32_lds_wave<MODE, MI, NT>(acc, bias, reinterpret_cast<float*>(out), N, m0 + wm * WROWS,
                                            n0 + wn * 64, lane, smem + wave * 16384);
    }
}

// ------------------------------------------------------------------------------------------------
// The 3x3 convolution (conv3x3_kernel above) on the ping-pong kernel's tile, ring and schedule: 256 x 256 output
// tile, K-tiles of 32 input channels of one tap (Cin % 32 == 0).  Only the A
// staging differs from gemm_pp_kernel: the two (or, never here, three) rows a lane stages keep their (t, f) coordinates
// in registers, the tap of the K-tile being staged shifts the source address, and a row whose neighbour lies outside
// the image reads the page of zeros.  Same vmcnt counts (same number of LDS-DMA instructions per K-tile), same RAW / WAR
// argument.  out has ceil256(M) rows.
// ------------------------------------------------------------------------------------------------
// POOL: as in conv3x3_kernel — row wm*128 + i*16 + l is member i & 3 of the window of output cell
// 64*tile + 32*wm + 16*(i >> 2) + l, so a window is acc[4h .. 4h+3][j] of one lane.
template <bool POOL>
__global__ __launch_bounds__(512, 2) void conv3x3_pp_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ Wt,
                                                            const float* __restrict__ bias,
                                                            const bf16_t* __restrict__ zeros, int T, int F, int Cin,
                                                            int M, int Cout, bf16_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int BKT = 32, NT = 4, WROWS = 128, MI = WROWS / 16;
    constexpr int BMB = 256;
    constexpr int WM_WAVES = BMB / WROWS, WN_WAVES = 8 / WM_WAVES, BNB = WN_WAVES * 64;
    constexpr int STAGES = 4;
    constexpr int TA = BMB * BKT * 2, TBt = BNB * BKT * 2, SB = TA + TBt;
    constexpr int GPS = TA / 8192 + TBt / 8192;
    constexpr int INFL = (STAGES - 2) * GPS;
    constexpr int RA = TA / 8192;                      // A rows a lane stages (2)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int wm = wave / WN_WAVES, wn = wave % WN_WAVES;
    const bool late = __builtin_amdgcn_readfirstlane(threadIdx.x) >= 256;

    const int tiles_n = Cout / BNB;
    int tm, tn;
    tile_coords((M + BMB - 1) / BMB, tiles_n, 4, &tm, &tn);
    const int m0 = tm * BMB, n0 = tn * BNB;
    const int K = 9 * Cin, ck = Cin / BKT, nk = 9 * ck;

    int pt[RA], pf[RA];
    long long poff[RA];
    const int T2 = T >> 1, F2 = F >> 1;
    const int base = POOL ? tm * 64 : m0;
    const CellBase cb = POOL ? cell_base(base, T2, F2, 63) : cell_base(base, T, F, BMB - 1);
#pragma unroll
    for (int t = 0; t < RA; ++t) {
        const int r = (t * 8 + wave) * 16 + (lane >> 2);
        const int c = swz_chunk<BKT>(r, lane & 3);
        if constexpr (POOL) {
            const int i = (r >> 4) & 7, mem = i & 3;
            const int local = (r >> 7) * 32 + (i >> 2) * 16 + (r & 15);
            int b, t2, f2;
            cell_at(cb, base, local, T2, F2, &b, &t2, &f2);
            const int tt = 2 * t2 + (mem >> 1), ff = 2 * f2 + (mem & 1);
            pf[t] = ff;
            pt[t] = (4 * (base + local) < M) ? tt : -4;
            poff[t] = ((long long)(b * T + tt) * F + ff) * Cin + c * 8;
        } else {
            int b, tt, ff;
            cell_at(cb, base, r, T, F, &b, &tt, &ff);
            pf[t] = ff;
            pt[t] = (m0 + r < M) ? tt : -4;
            poff[t] = (long long)(m0 + r) * Cin + c * 8;
        }
    }
    int tap = 0, cc = 0;                               // of the K-tile staged next
    auto stage_next = [&](int kt_stage, unsigned char* dst) {
        const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
        const long long shift = (long long)(dy * F + dx) * Cin + cc * BKT;
#pragma unroll
        for (int t = 0; t < RA; ++t) {
            const bool in = (unsigned)(pt[t] + dy) < (unsigned)T && (unsigned)(pf[t] + dx) < (unsigned)F;
            glds16(in ? X + poff[t] + shift : zeros, dst + (t * 8 + wave) * 1024);
        }
        stage_rows8_ring<BNB, BKT>(Wt, K, n0, kt_stage * BKT, dst + TA, wave, lane);
        if (++cc == ck) { cc = 0; ++tap; }
    };

    f32x4 acc[MI][NT];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int s = 0; s < STAGES - 1; ++s)
        if (s < nk) stage_next(s, smem + s * SB);       // nk >= 18 > STAGES - 1 always (Cin >= 64)
    if (late) {
        wait_vmcnt<INFL>();
        __builtin_amdgcn_s_barrier();
    }
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + STAGES - 2 < nk) wait_vmcnt<INFL>(); else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (kt + STAGES - 1 < nk) {
            int ns = cur + STAGES - 1;
            if (ns >= STAGES) ns -= STAGES;
            stage_next(kt + STAGES - 1, smem + ns * SB);
        }
        const unsigned char* At = smem + cur * SB;
        const unsigned char* Bt = At + TA;
        const int chunk = lane >> 4;
        bf16x8 wf[NT], af[MI];
#pragma unroll
        for (int j = 0; j < NT; ++j) wf[j] = lds_frag_ring<BKT>(Bt, wn * 64 + j * 16 + (lane & 15), chunk);
#pragma unroll
        for (int i = 0; i < MI; ++i) af[i] = lds_frag_ring<BKT>(At, wm * WROWS + i * 16 + (lane & 15), chunk);
        if (kt + STAGES - 1 < nk) wait_vmcnt<INFL>(); else wait_vmcnt<0>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        cur = (cur + 1 == STAGES) ? 0 : cur + 1;
    }
    if (!late) __builtin_amdgcn_s_barrier();
    if constexpr (POOL) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int q = tm * 64 + wm * 32 + h * 16 + (lane & 15);
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int n = n0 + wn * 64 + j * 16 + (lane >> 4) * 4;
                const float4 bv = *reinterpret_cast<const float4*>(bias + n);
                float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
#pragma unroll
                for (int i = 4 * h; i < 4 * h + 4; ++i) {
                    v0 += fmaxf(acc[i][j][0] + bv.x, 0.f); v1 += fmaxf(acc[i][j][1] + bv.y, 0.f);
                    v2 += fmaxf(acc[i][j][2] + bv.z, 0.f); v3 += fmaxf(acc[i][j][3] + bv.w, 0.f);
                }
                uint2 pk;
                pk.x = pack_bf16x2(0.25f * v0, 0.25f * v1);
                pk.y = pack_bf16x2(0.25f * v2, 0.25f * v3);
                if (4 * q < M) *reinterpret_cast<uint2*>(out + (size_t)q * Cout + n) = pk;
            }
        }
        return;
    }
    __syncthreads();  // both groups are past their last fragment read: the ring is dead
    epilogue_big_lds<EPI_RELU, MI>(acc, bias, out, Cout, m0, n0, wm, wn, lane, wave, smem);
}


template <int MODE, int WROWS>
static void launch_pp(const bf16_t* A, const bf16_t* Wt, const float* bias, int M, int N, int K, void* out,
                      hipStream_t st) {
    auto kern = gemm_pp_kernel<MODE, WROWS>;
    constexpr int BNB = (WROWS == 80) ? 128 : 256;
    constexpr int BMB = (WROWS == 80) ? 320 : 2 * WROWS;
    const size_t lds = (size_t)4 * (BMB + BNB) * 32 * 2;  // 128 KiB / 112 KiB / 144 KiB
    static PerDeviceOnce attr_set;
    attr_set([&] {
        raise_lds_limit(reinterpret_cast<const void*>(kern), (int)lds);
    });
    const int grid = (M / BMB) * (N / BNB);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, A, Wt, bias, M, N, K, out);
}

#ifdef WISE_DEBUG_KNOBS
static int g_gemm_variant = 0;   // wise_debug_set_gemm_variant: a variant id forced for A/B runs (tools/gemm_bench.py)
#else
constexpr int g_gemm_variant = 0;
#endif
static thread_local int g_overlapped = 0;  // the calling thread is running another stream's kernels beside this one (gemm_set_overlapped)

// compute units of the current device (the persistent kernel's grid), asked once per device
static int device_cus() {
    static int cus[16] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 16) return 256;
    if (cus[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev] = n;
    }
    return cus[dev];
}

// launches variant v as resolve_variant() returned it (the shape fits)
template <int MODE>
static void launch_variant(int v, const bf16_t* A, const bf16_t* Wt, const float* bias, int M, int N, int K,
                           void* out, hipStream_t st) {
    switch (v) {
        case 1: launch_ring<MODE, 32, 4, 2>(A, Wt, bias, M, N, K, out, st); break;
        case 2: launch_ring<MODE, 64, 4, 1>(A, Wt, bias, M, N, K, out, st); break;   // skinny problems: 4 K-tiles of 64 in flight per block
        case 5: launch_big<MODE, 3>(A, Wt, bias, M, N, K, out, st); break;
        case 40: launch_pp<MODE, 128>(A, Wt, bias, M, N, K, out, st); break;
        case 42: launch_pp<MODE, 160>(A, Wt, bias, M, N, K, out, st); break;
        case 44: launch_pp<MODE, 80>(A, Wt, bias, M, N, K, out, st); break;
        case 60: launch_w4<MODE, 8, 8, 3, 2>(A, Wt, bias, M, N, K, out, st); break;
        case 61: launch_w4<MODE, 5, 8, 3, 2>(A, Wt, bias, M, N, K, out, st); break;
        case 62: if constexpr (bf16_out(MODE)) launch_w4<MODE, 10, 8, 2, 2>(A, Wt, bias, M, N, K, out, st); break;
        case 63: if constexpr (bf16_out(MODE)) launch_w4<MODE, 10, 6, 2, 3>(A, Wt, bias, M, N, K, out, st); break;
        case 64: if constexpr (bf16_out(MODE)) launch_w4p<MODE>(A, Wt, bias, M, N, K, out, device_cus(), st); break;
        case 65: launch_w4<MODE, 7, 6, 3, 2>(A, Wt, bias, M, N, K, out, st); break;
        case 66: launch_w4<MODE, 8, 6, 3, 2>(A, Wt, bias, M, N, K, out, st); break;
        case 67: launch_w4<MODE, 4, 6, 3, 2>(A, Wt, bias, M, N, K, out, st); break;
        case 68: launch_w4<MODE, 4, 8, 3, 2>(A, Wt, bias, M, N, K, out, st); break;
        // (69, 70: two workgroups per CU, 80 KiB of LDS: one workgroup's prologue and epilogue run under the other's K-loop)
        case 69: launch_w4<MODE, 4, 6, 2, 2, 2>(A, Wt, bias, M, N, K, out, st); break;
        case 70: launch_w4<MODE, 4, 4, 3, 2, 2>(A, Wt, bias, M, N, K, out, st); break;
        default: launch_gemm<MODE>(A, Wt, bias, M, N, K, out, st); break;
    }
}

static int launch_mode(int v, const bf16_t* A, const bf16_t* Wt, const float* bias, int M, int N, int K, int mode,
                       void* out, hipStream_t st) {
    switch (mode) {
        case EPI_BF16: launch_variant<EPI_BF16>(v, A, Wt, bias, M, N, K, out, st); break;
        case EPI_QUICKGELU: launch_variant<EPI_QUICKGELU>(v, A, Wt, bias, M, N, K, out, st); break;
        case EPI_GELU: launch_variant<EPI_GELU>(v, A, Wt, bias, M, N, K, out, st); break;
        case EPI_GELU_TANH: launch_variant<EPI_GELU_TANH>(v, A, Wt, bias, M, N, K, out, st); break;
        case EPI_RELU: launch_variant<EPI_RELU>(v, A, Wt, bias, M, N, K, out, st); break;
        case EPI_RESID: launch_variant<EPI_RESID>(v, A, Wt, bias, M, N, K, out, st); break;
        case EPI_F32: launch_variant<EPI_F32>(v, A, Wt, bias, M, N, K, out, st); break;
        default: set_error("gemm_bf16: unknown mode %d", mode); return WISE_E_INVALID;
    }
    WISE_LAUNCH_CHECK("gemm_bf16_kernel");
    return WISE_OK;
}

// the tiled launches of a plan, one after the other on the stream
static int launch_tiles(const GemmPlan& p, const bf16_t* A, const bf16_t* Wt, const float* bias, int N, int K, int mode,
                        void* out, hipStream_t st) {
    int M = 0;
    for (int i = 0; i < p.n; ++i) M += p.rows[i];
    ProfScope prof(PROF_GEMM, 2.0 * (double)M * (double)N * (double)K, st);
    const size_t esz = (mode == EPI_RESID || mode == EPI_F32) ? 4 : 2;
    for (int i = 0, m0 = 0; i < p.n; m0 += p.rows[i], ++i)
        if (const int rc = launch_mode(p.v[i], A + (size_t)m0 * K, Wt, bias, p.rows[i], N, K, mode,
                                       reinterpret_cast<unsigned char*>(out) + (size_t)m0 * N * esz, st))
            return rc;
    return WISE_OK;
}

void gemm_set_overlapped(bool on) { g_overlapped = on ? 1 : 0; }

// x[M,96] += fc2(gelu(fc1(LN(x)))) in one kernel; M % 128 == 0 (rows readable and writable)
int mlp96_fused(float* x, const float* lnw, const float* lnb, const bf16_t* W1, const float* b1, const bf16_t* W2,
                const float* b2, int M, float eps, hipStream_t st) {
    WISE_CHECK_ARG(x && lnw && lnb && W1 && b1 && W2 && b2 && M > 0 && M % 128 == 0, "mlp96: bad argument (M=%d)", M);
    ProfScope prof(PROF_GEMM, 4.0 * (double)M * 96.0 * 384.0, st);
    const size_t ldsr = (size_t)MLPR_W1_BYTES + MLPR_W2_BYTES + (384 + 3 * 96) * sizeof(float);   // 150 KiB
    static PerDeviceOnce attr_r;
    attr_r([&] {
        raise_lds_limit(reinterpret_cast<const void*>(mlp96r_kernel), (int)ldsr);
    });
    const long long units = M / 32;
    const int grid = units < 8 * 256 ? (int)((units + 7) / 8) : 256;
    hipLaunchKernelGGL(mlp96r_kernel, dim3(grid), dim3(512), ldsr, st, x, lnw, lnb, W1, b1, W2, b2, units, eps);
    WISE_LAUNCH_CHECK("mlp96r_kernel");
    return WISE_OK;
}

bool gemm_ln_supported(int N, int K, int mode) { return (K == 96 || K == 192) && N % 8 == 0 && bf16_out(mode); }

// out_bf16[M,N] = epi( LayerNorm(x[M,K]; lnw, lnb, eps) @ Wt^T + bias ); M % 128 == 0 (rows readable), K in {96, 192}
int gemm_ln_bf16(const float* x, const float* lnw, const float* lnb, const bf16_t* Wt, const float* bias, int M, int N,
                 int K, float eps, int mode, bf16_t* out, hipStream_t st) {
    WISE_CHECK_ARG(x && lnw && lnb && Wt && out, "gemm_ln: null pointer");
    WISE_CHECK_ARG(M > 0 && M % 128 == 0 && gemm_ln_supported(N, K, mode), "gemm_ln: M=%d N=%d K=%d mode=%d unsupported", M,
                   N, K, mode);
    ProfScope prof(PROF_GEMM, 2.0 * (double)M * (double)N * (double)K, st);
#define LN_CASE(MD)                                                                          \
    case MD:                                                                                 \
        if (K == 96) launch_gemm_ln<MD, 3>(x, lnw, lnb, Wt, bias, M, N, eps, out, st);        \
        else launch_gemm_ln<MD, 6>(x, lnw, lnb, Wt, bias, M, N, eps, out, st);                \
        break;
    switch (mode) {
        LN_CASE(EPI_BF16) LN_CASE(EPI_QUICKGELU) LN_CASE(EPI_GELU) LN_CASE(EPI_GELU_TANH)
        default: set_error("gemm_ln: mode %d", mode); return WISE_E_INVALID;
    }
#undef LN_CASE
    WISE_LAUNCH_CHECK("gemm_ln_kernel");
    return WISE_OK;
}

template <int MODE>
static void launch_reduce(const float* part, int S, int rows, int N, const float* bias, void* out, hipStream_t st) {
    const int total = rows * (N / 4);
    hipLaunchKernelGGL(splitk_reduce_kernel<MODE>, dim3((total + 255) / 256), dim3(256), 0, st, part, S, rows, N, bias, out);
}

size_t gemm_splitk_bytes(int M, int m_valid, int N, int K) {
    return (size_t)splitk_slices(M, m_valid, N, K) * 128 * (size_t)N * sizeof(float);
}
static void splitk_partials(const bf16_t* A, const bf16_t* Wt, int N, int K, int S, float* part, hipStream_t st) {
    constexpr int STAGES = 4;
    const size_t lds = (size_t)STAGES * 2 * 128 * 64 * 2;
    static PerDeviceOnce attr_set;
    attr_set([&] {
        raise_lds_limit(reinterpret_cast<const void*>(gemm_splitk_kernel<STAGES>), (int)lds);
    });
    hipLaunchKernelGGL(gemm_splitk_kernel<STAGES>, dim3(N / 128, S), dim3(256), lds, st, A, Wt, N, K, K / S, part);
}

// rows 0..m_valid-1 (<= 128) of A @ Wt^T through the split-K pair of kernels, S slices of K, the partials in the caller's
// fp32 scratch `part`; false = the scratch is missing or too small for this call.
static bool gemm_splitk(const bf16_t* A, const bf16_t* Wt, const float* bias, int S, int m_valid, int N, int K, int mode,
                        void* out, hipStream_t st, float* part, size_t part_bytes) {
    if (!part || part_bytes < (size_t)S * 128 * N * sizeof(float)) return false;
    ProfScope prof(PROF_GEMM, 2.0 * (double)m_valid * (double)N * (double)K, st);
    splitk_partials(A, Wt, N, K, S, part, st);
    switch (mode) {
        case EPI_BF16: launch_reduce<EPI_BF16>(part, S, m_valid, N, bias, out, st); break;
        case EPI_QUICKGELU: launch_reduce<EPI_QUICKGELU>(part, S, m_valid, N, bias, out, st); break;
        case EPI_GELU: launch_reduce<EPI_GELU>(part, S, m_valid, N, bias, out, st); break;
        case EPI_GELU_TANH: launch_reduce<EPI_GELU_TANH>(part, S, m_valid, N, bias, out, st); break;
        case EPI_RELU: launch_reduce<EPI_RELU>(part, S, m_valid, N, bias, out, st); break;
        case EPI_RESID: launch_reduce<EPI_RESID>(part, S, m_valid, N, bias, out, st); break;
        default: launch_reduce<EPI_F32>(part, S, m_valid, N, bias, out, st); break;
    }
    return true;
}

// m_valid: the rows of A that carry data (the rest of the M rows are padding whose results nobody reads)
int gemm_bf16_rows(const bf16_t* A, const bf16_t* Wt, const float* bias, int M, int m_valid, int N, int K, int mode,
                   void* out, hipStream_t st, float* sk, size_t sk_bytes) {
    WISE_CHECK_ARG(A && Wt && out, "gemm_bf16: null pointer");
    WISE_CHECK_ARG(M > 0 && M % BM == 0 && N > 0 && N % 4 == 0 && K > 0 && K % 32 == 0 && mode >= 0 && mode <= 6,
                   "gemm_bf16: M=%d must be a multiple of %d, N=%d of 4, K=%d of 32", M, BM, N, K);
    const GemmPlan p = gemm_plan(M, N, K, mode, m_valid, g_overlapped != 0, device_cus(), g_gemm_variant);
    if (p.splitk && gemm_splitk(A, Wt, bias, p.splitk, m_valid, N, K, mode, out, st, sk, sk_bytes)) {
        WISE_LAUNCH_CHECK("gemm_splitk_kernel");
        return WISE_OK;
    }
    return launch_tiles(p, A, Wt, bias, N, K, mode, out, st);
}

// x[M,N] += A @ Wt^T + bias (the residual GEMM of a block), then the LayerNorm that follows it: h = LN(x) as bf16, and for
// post-LN blocks (post_ln) x = LN(x) as well.  Skinny calls (the text towers' single queries) run the split-K partial
// kernel and ONE kernel for reduction + residual + LayerNorm; everything else is the two launches it stands for.
// The same bits either way, x and h (and the normalised x of post_ln): the reduction adds in the split-K residual GEMM's
// order and the fused kernel sums the row's statistics in layernorm_kernel's (tests/test_gpu_gemm_skinny.py holds both to
// it).  It used not to: with the statistics summed per wave and then over the four waves, mean and rstd had other last bits,
// a few elements in 10^5 of h landed on the neighbouring bf16 value, and one that ln_b cancelled to 9e-7 four values away.
// The LayerNorm's width is checked here, before the first launch: a refused call leaves x as it was.
int gemm_resid_ln_rows(const bf16_t* A, const bf16_t* Wt, const float* bias, int M, int m_valid, int ln_rows, int N, int K,
                       float* x, const float* ln_w, const float* ln_b, float eps, bool post_ln, bf16_t* h, hipStream_t st,
                       float* sk, size_t sk_bytes) {
    WISE_CHECK_ARG(A && Wt && x && ln_w && ln_b && h, "gemm_resid_ln: null pointer");
    WISE_CHECK_ARG(N >= 4 && N % 4 == 0 && N <= 4096 && (!post_ln || N > 128),
                   "gemm_resid_ln: N=%d must be a multiple of 4, <= 4096%s", N, post_ln ? " and > 128 (post-LN)" : "");
    // (ln_rows: the rows the LayerNorm covers — the caller's real rows; m_valid may include tile padding.  The fused
    // reduction holds a row of up to 4096 columns.)
    const GemmPlan p = gemm_plan(M, N, K, EPI_RESID, m_valid, g_overlapped != 0, device_cus(), g_gemm_variant);
    const int S = (N > 128 && N <= 4096 && ln_rows == m_valid) ? p.splitk : 0;
    float* part = (S && sk && sk_bytes >= (size_t)S * 128 * N * sizeof(float)) ? sk : nullptr;
    if (part) {
        {
            ProfScope prof(PROF_GEMM, 2.0 * (double)m_valid * (double)N * (double)K, st);
            splitk_partials(A, Wt, N, K, S, part, st);
        }
        with_nv<4>((N / 4 + 255) / 256, [&](auto n) {      // (float4s per THREAD here: N <= 4096)
            hipLaunchKernelGGL(splitk_reduce_ln_kernel<decltype(n)::value>, dim3(m_valid), dim3(256), 0, st, part, S, m_valid, N, bias,
                               x, ln_w, ln_b, eps, h, post_ln ? 1 : 0);
        });
        WISE_LAUNCH_CHECK("splitk_reduce_ln_kernel");
        return WISE_OK;
    }
    int rc;
    if ((rc = gemm_bf16_rows(A, Wt, bias, M, m_valid, N, K, EPI_RESID, x, st, sk, sk_bytes))) return rc;
    return post_ln ? layernorm_f32_dual(x, ln_w, ln_b, ln_rows, N, eps, x, h, st) : layernorm_f32_bf16(x, ln_w, ln_b, ln_rows, N, eps, h, st);
}

int gemm_bf16(const bf16_t* A, const bf16_t* Wt, const float* bias, int M, int N, int K, int mode, void* out,
              hipStream_t st) {
    WISE_CHECK_ARG(A && Wt && out, "gemm_bf16: null pointer");
    WISE_CHECK_ARG(M > 0 && M % BM == 0 && N > 0 && N % 4 == 0 && K > 0 && K % 32 == 0,
                   "gemm_bf16: M=%d must be a multiple of %d, N=%d of 4, K=%d of 32", M, BM, N, K);
    return launch_tiles(gemm_plan(M, N, K, mode, 0, g_overlapped != 0, device_cus(), g_gemm_variant), A, Wt, bias, N, K,
                        mode, out, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// The two GEMM forms of the LayerNorm fold (gemm_w4.h FoldArgs; vit.hip's fold mode): every one of them is a one-wave-per-
// SIMD kernel, whose epilogues live in ONE place, so a row gets the same bits from whatever tile its batch size selects.
//   consumer:  out bf16 [M,N] = act(rstd[row] * (A @ Wt^T) + bias[col])          (QKV, fc1; A = bf16 copy of the residual rows)
//   producer:  x += A @ Wt^T + bias;  h = bf16(x);  part / rstd_out = the rows' statistics    (out-projection, fc2)
// M % 128 == 0, N % 128 == 0, K % 64 == 0, K >= 192.  Tiles with 64- or 128-column wave parts only (the statistics' tree).
// ---------------------------------------------------------------------------------------------------------------------
bool gemm_fold_shape_ok(int M, int N, int K) { return M > 0 && M % 128 == 0 && N > 0 && (N % 128 == 0 || N % 192 == 0) && K % 64 == 0 && K >= 192; }

template <int MODE>
static void launch_fold_consumer(int v, const bf16_t* A, const bf16_t* Wt, const float* bias, int M, int N, int K, bf16_t* out,
                                 const FoldArgs& fa, hipStream_t st) {
    switch (v) {
        case 60: launch_w4<MODE, 8, 8, 3, 2, 1, 1>(A, Wt, bias, M, N, K, out, st, fa); break;
        case 61: launch_w4<MODE, 5, 8, 3, 2, 1, 1>(A, Wt, bias, M, N, K, out, st, fa); break;
        case 64: launch_w4p<MODE, 1>(A, Wt, bias, M, N, K, out, device_cus(), st, fa); break;
        case 68: launch_w4<MODE, 4, 8, 3, 2, 1, 1>(A, Wt, bias, M, N, K, out, st, fa); break;
        case 66: launch_w4<MODE, 8, 6, 3, 2, 1, 1>(A, Wt, bias, M, N, K, out, st, fa); break;
        case 67: launch_w4<MODE, 4, 6, 3, 2, 1, 1>(A, Wt, bias, M, N, K, out, st, fa); break;
        case 69: launch_w4<MODE, 4, 6, 2, 2, 2, 1>(A, Wt, bias, M, N, K, out, st, fa); break;
        default: launch_w4<MODE, 4, 4, 3, 2, 2, 1>(A, Wt, bias, M, N, K, out, st, fa); break;
    }
}

int gemm_fold_bf16(const bf16_t* A, const bf16_t* Wt, const float* bias, const float* rstd, int M, int N, int K, int mode,
                   bf16_t* out, hipStream_t st) {
    WISE_CHECK_ARG(A && Wt && bias && rstd && out, "gemm_fold_bf16: null pointer");
    WISE_CHECK_ARG(gemm_fold_shape_ok(M, N, K) && bf16_out(mode) && mode != EPI_RELU, "gemm_fold_bf16: M=%d N=%d K=%d mode=%d", M, N, K, mode);
    ProfScope prof(PROF_GEMM, 2.0 * (double)M * (double)N * (double)K, st);
    FoldArgs fa;
    fa.stats = const_cast<float*>(rstd);
    const int v = fold_plan(M, N, K, mode, false, false, device_cus());
    WISE_CHECK_ARG(v != 0, "gemm_fold_bf16: no tile for M=%d N=%d K=%d", M, N, K);
    switch (mode) {
        case EPI_BF16: launch_fold_consumer<EPI_BF16>(v, A, Wt, bias, M, N, K, out, fa, st); break;
        case EPI_QUICKGELU: launch_fold_consumer<EPI_QUICKGELU>(v, A, Wt, bias, M, N, K, out, fa, st); break;
        case EPI_GELU: launch_fold_consumer<EPI_GELU>(v, A, Wt, bias, M, N, K, out, fa, st); break;
        default: launch_fold_consumer<EPI_GELU_TANH>(v, A, Wt, bias, M, N, K, out, fa, st); break;
    }
    WISE_LAUNCH_CHECK("gemm_w4_kernel (fold, bf16 out)");
    return WISE_OK;
}

size_t gemm_fold_stats_bytes(int M, int N) { return fold_stats_bytes(M, N); }
size_t gemm_fold_counters_bytes(int M) { return fold_count_slots(M) * 4; }

template <int MODE>
static void launch_fold_producer(int v, const bf16_t* A, const bf16_t* Wt, const float* bias, int M, int N, int K, const FoldArgs& fa,
                                 hipStream_t st) {
    float* x = nullptr;
    switch (v) {
        case 61: if constexpr (MODE == EPI_RESID) { launch_w4<MODE, 5, 8, 3, 2, 1, 2>(A, Wt, bias, M, N, K, x, st, fa); break; }
        case 68: launch_w4<MODE, 4, 8, 3, 2, 1, 2>(A, Wt, bias, M, N, K, x, st, fa); break;
        case 66: launch_w4<MODE, 8, 6, 3, 2, 1, 2>(A, Wt, bias, M, N, K, x, st, fa); break;
        case 67: launch_w4<MODE, 4, 6, 3, 2, 1, 2>(A, Wt, bias, M, N, K, x, st, fa); break;
        case 69: launch_w4<MODE, 4, 6, 2, 2, 2, 2>(A, Wt, bias, M, N, K, x, st, fa); break;
        default: launch_w4<MODE, 4, 4, 3, 2, 2, 2>(A, Wt, bias, M, N, K, x, st, fa); break;
    }
}

// accumulate: x += ... (the residual GEMM of a block); otherwise x = ... (the rows that START a hi + lo stream: MS-CLAP HTSAT's
// patch-merging projection in front of a stage)
int gemm_fold_resid(const bf16_t* A, const bf16_t* Wt, const float* bias, int M, int N, int K, bf16_t* hi, long long lo_off,
                    float* stats, float eps, hipStream_t st, int group32, bool accumulate) {
    WISE_CHECK_ARG(A && Wt && hi && stats, "gemm_fold_resid: null pointer");
    WISE_CHECK_ARG(gemm_fold_shape_ok(M, N, K) && (group32 || N % 128 == 0), "gemm_fold_resid: M=%d N=%d K=%d group32=%d", M, N, K, group32);
    // lo sits BEHIND hi, within the 2 GiB a buffer descriptor's scalar offset reaches (the residual prefetch addresses it so)
    WISE_CHECK_ARG(lo_off >= (long long)M * N && lo_off % 4 == 0 && (lo_off + (long long)M * N) * 2 < 0x7fffffffLL,
                   "gemm_fold_resid: lo must follow hi by at least M*N elements and stay within 2 GiB of it (lo_off=%lld)", lo_off);
    ProfScope prof(PROF_GEMM, 2.0 * (double)M * (double)N * (double)K, st);
    FoldArgs fa;
    fa.hcopy = hi; fa.lo_off = (int)lo_off; fa.stats = stats; fa.eps = eps; fa.group32 = group32 ? 1 : 0;
    const int v = fold_plan(M, N, K, accumulate ? EPI_RESID : EPI_F32, true, group32 != 0, device_cus());
    WISE_CHECK_ARG(v != 0, "gemm_fold_resid: no tile for M=%d N=%d K=%d", M, N, K);
    if (accumulate) launch_fold_producer<EPI_RESID>(v, A, Wt, bias, M, N, K, fa, st);
    else launch_fold_producer<EPI_F32>(v, A, Wt, bias, M, N, K, fa, st);
    WISE_LAUNCH_CHECK("gemm_w4_kernel (fold, residual)");
    return WISE_OK;
}

template <typename K>
static void conv_launch(K kern, size_t lds, int grid, int threads, const bf16_t* X, const bf16_t* Wt, const float* bias,
                        const bf16_t* zeros, int T, int F, int Cin, int M, int Cout, bf16_t* out, hipStream_t st) {
    static std::mutex mu;
    static std::vector<std::pair<const void*, int>> configured;   // (kernel, device) whose dynamic-LDS limit has been raised
    {
        std::lock_guard<std::mutex> lk(mu);
        int dev = 0;
        (void)hipGetDevice(&dev);
        const std::pair<const void*, int> id(reinterpret_cast<const void*>(kern), dev);
        bool seen = false;
        for (const auto& c : configured) seen = seen || c == id;
        if (!seen) {
            raise_lds_limit(id.first, (int)lds);
            configured.push_back(id);
        }
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, st, X, Wt, bias, zeros, T, F, Cin, M, Cout, out);
}

// relu(conv3x3(X [B, T, F, Cin] bf16 NHWC) + bias), Cin % 64 == 0, Cout % 64 == 0:
//   pool == false: out [ceil256(B*T*F), Cout] bf16 (rows padded to the tile)
//   pool == true:  avg_pool2d(., 2) (floor) of it, out [B*(T/2)*(F/2), Cout] bf16 — the full-resolution tensor is never written
// `zeros`: at least 16 readable bytes of zeros on the device (the padding every out-of-image tap reads).
int conv3x3_bf16(const bf16_t* X, const bf16_t* Wt, const float* bias, const bf16_t* zeros, int B, int T, int F, int Cin,
                 int Cout, bool pool, bf16_t* out, hipStream_t st) {
    WISE_CHECK_ARG(X && Wt && bias && zeros && out, "conv3x3: null pointer");
    WISE_CHECK_ARG(B > 0 && T > 0 && F > 0 && Cin > 0 && Cin % 64 == 0 && Cout > 0 && Cout % 64 == 0 && (!pool || (T >= 2 && F >= 2)),
                   "conv3x3: B=%d T=%d F=%d Cin=%d Cout=%d unsupported", B, T, F, Cin, Cout);
    const long long M = conv_rows(B, T, F, pool);
    WISE_CHECK_ARG((long long)B * T * F * (long long)(Cin > Cout ? Cin : Cout) < (1ll << 40) && (long long)B * T * F < (1ll << 31) - 256,
                   "conv3x3: B=%d T=%d F=%d too large", B, T, F);
    ProfScope prof(PROF_GEMM, 2.0 * (double)M * (double)Cout * 9.0 * (double)Cin, st);
    const int tiles256 = (int)((M + 255) / 256), tiles_m = (int)((M + 127) / 128);
    switch (conv_plan(M, Cout)) {
        case CONV_PP256: {
            const size_t lds = (size_t)4 * (256 + 256) * 64;   // 128 KiB
            const int grid = tiles256 * (Cout / 256);
            if (pool) conv_launch(conv3x3_pp_kernel<true>, lds, grid, 512, X, Wt, bias, zeros, T, F, Cin, (int)M, Cout, out, st);
            else conv_launch(conv3x3_pp_kernel<false>, lds, grid, 512, X, Wt, bias, zeros, T, F, Cin, (int)M, Cout, out, st);
            WISE_LAUNCH_CHECK("conv3x3_pp_kernel");
            return WISE_OK;
        }
        case CONV_128x128: {
            const size_t lds = 2 * (TILE_BYTES + 128 * BK * 2);   // 64 KiB
            if (pool) conv_launch(conv3x3_kernel<4, true>, lds, tiles_m * (Cout / 128), 256, X, Wt, bias, zeros, T, F, Cin, (int)M, Cout, out, st);
            else conv_launch(conv3x3_kernel<4, false>, lds, tiles_m * (Cout / 128), 256, X, Wt, bias, zeros, T, F, Cin, (int)M, Cout, out, st);
            break;
        }
        case CONV_256x64: {
            const size_t lds = 2 * (2 * TILE_BYTES + 64 * BK * 2);    // 80 KiB: two blocks fill a CU's LDS exactly
            if (pool) conv_launch(conv3x3_kernel<4, true, 4>, lds, tiles256 * (Cout / 64), 256, X, Wt, bias, zeros, T, F, Cin, (int)M, Cout, out, st);
            else conv_launch(conv3x3_kernel<4, false, 4>, lds, tiles256 * (Cout / 64), 256, X, Wt, bias, zeros, T, F, Cin, (int)M, Cout, out, st);
            break;
        }
        case CONV_128x64: {
            const size_t lds = 2 * (TILE_BYTES + 64 * BK * 2);    // 48 KiB
            if (pool) conv_launch(conv3x3_kernel<2, true>, lds, tiles_m * (Cout / 64), 256, X, Wt, bias, zeros, T, F, Cin, (int)M, Cout, out, st);
            else conv_launch(conv3x3_kernel<2, false>, lds, tiles_m * (Cout / 64), 256, X, Wt, bias, zeros, T, F, Cin, (int)M, Cout, out, st);
            break;
        }
    }
    WISE_LAUNCH_CHECK("conv3x3_kernel");
    return WISE_OK;
}

}  // namespace wise

extern "C" int wise_mlp96_fused(float* x, const float* lnw, const float* lnb, const uint16_t* W1, const float* b1,
                                const uint16_t* W2, const float* b2, int M, float eps, void* stream) {
    return wise::mlp96_fused(x, lnw, lnb, W1, b1, W2, b2, M, eps, (hipStream_t)stream);
}

extern "C" int wise_gemm_ln_bf16(const float* x, const float* lnw, const float* lnb, const uint16_t* Wt, const float* bias,
                                 int M, int N, int K, float eps, int mode, uint16_t* out, void* stream) {
    return wise::gemm_ln_bf16(x, lnw, lnb, Wt, bias, M, N, K, eps, mode, out, (hipStream_t)stream);
}

extern "C" void wise_overlap_hint(int on) { wise::gemm_set_overlapped(on != 0); }

extern "C" size_t wise_gemm_fold_stats_bytes(int M, int N) { return wise::gemm_fold_shape_ok(M, N, 192) ? wise::gemm_fold_stats_bytes(M, N) : 0; }
extern "C" size_t wise_gemm_fold_counters_offset(int M) { return (size_t)M * 4; }
extern "C" size_t wise_gemm_fold_counters_bytes(int M) { return wise::fold_count_slots(M) * 4; }
extern "C" int wise_gemm_fold_bf16(const uint16_t* A, const uint16_t* Wt, const float* bias, const float* rstd, int M, int N, int K,
                                   int mode, uint16_t* out, void* stream) {
    return wise::gemm_fold_bf16(A, Wt, bias, rstd, M, N, K, mode, out, (hipStream_t)stream);
}
extern "C" int wise_gemm_fold_resid(const uint16_t* A, const uint16_t* Wt, const float* bias, int M, int N, int K, uint16_t* hi,
                                    int64_t lo_off, float* stats, float eps, int group32, void* stream) {
    return wise::gemm_fold_resid(A, Wt, bias, M, N, K, hi, lo_off, stats, eps, (hipStream_t)stream, group32 & 1, !(group32 & 2));
}

extern "C" int wise_gemm_bf16(const uint16_t* A, const uint16_t* Wt, const float* bias, int M, int N, int K, int mode,
                              void* out, void* stream) {
    return wise::gemm_bf16(A, Wt, bias, M, N, K, mode, out, (hipStream_t)stream);
}

#ifdef WISE_DEBUG_KNOBS
// tuning knob for A/B runs (tools/gemm_bench.py); not part of the stable ABI.  v & 0xFF: a variant id (0 = the plan's own
// choice) that every gemm_bf16 / gemm_bf16_rows call then launches, after the shape fallbacks of resolve_variant.
extern "C" int wise_debug_set_gemm_variant(int v) {
    wise::g_gemm_variant = v & 0xFF;
    return 0;
}

// The tile plan as ints, for tests/test_gemm_plan_cpu.py (no GPU needed).  Returns the number of ints written to out.
//   kind 0, gemm_plan:  a = M, N, K, mode, m_valid (0: gemm_bf16), overlapped, cus -> splitk, n, v0, rows0, v1, rows1
//   kind 1, fold_plan:  a = M, N, K, mode, producer, wide96, cus                     -> variant
//   kind 2, conv_plan:  a = B, T, F, Cin, Cout, pool                                 -> ConvTile
//   kind 3, gemm_plan under wise_debug_set_gemm_variant(force) (force = 0: the plan's own choice, as kind 0 with
//           m_valid = 0):  a = force, M, N, K, mode, cus                             -> as kind 0
extern "C" int wise_debug_gemm_plan(int kind, const int* a, int* out) {
    if (kind == 0) {
        const wise::GemmPlan p = wise::gemm_plan(a[0], a[1], a[2], a[3], a[4], a[5] != 0, a[6]);
        const int r[6] = {p.splitk, p.n, p.v[0], p.rows[0], p.v[1], p.rows[1]};
        for (int i = 0; i < 6; ++i) out[i] = r[i];
        return 6;
    }
    if (kind == 1) {
        out[0] = wise::fold_plan(a[0], a[1], a[2], a[3], a[4] != 0, a[5] != 0, a[6]);
        return 1;
    }
    if (kind == 3) {
        const wise::GemmPlan p = wise::gemm_plan(a[1], a[2], a[3], a[4], 0, false, a[5], a[0] & 0xFF);
        const int r[6] = {p.splitk, p.n, p.v[0], p.rows[0], p.v[1], p.rows[1]};
        for (int i = 0; i < 6; ++i) out[i] = r[i];
        return 6;
    }
    if (kind == 2) {
        out[0] = wise::conv_plan(wise::conv_rows(a[0], a[1], a[2], a[5] != 0), a[4]);
        return 1;
    }
    return 0;
}

// The skinny-GEMM entry points as the towers call them (m_valid rows of data, the caller's split-K scratch), for
// tests/test_gpu_gemm_skinny.py: the split-K pair and the fused reduction + LayerNorm have no other way in.
extern "C" size_t wise_debug_gemm_splitk_bytes(int M, int m_valid, int N, int K) { return wise::gemm_splitk_bytes(M, m_valid, N, K); }
extern "C" int wise_debug_gemm_rows(const uint16_t* A, const uint16_t* Wt, const float* bias, int M, int m_valid, int N, int K,
                                    int mode, void* out, float* sk, size_t sk_bytes, void* stream) {
    return wise::gemm_bf16_rows(A, Wt, bias, M, m_valid, N, K, mode, out, (hipStream_t)stream, sk, sk_bytes);
}
extern "C" int wise_debug_gemm_resid_ln_rows(const uint16_t* A, const uint16_t* Wt, const float* bias, int M, int m_valid,
                                             int ln_rows, int N, int K, float* x, const float* ln_w, const float* ln_b, float eps,
                                             int post_ln, uint16_t* h, float* sk, size_t sk_bytes, void* stream) {
    return wise::gemm_resid_ln_rows(A, Wt, bias, M, m_valid, ln_rows, N, K, x, ln_w, ln_b, eps, post_ln != 0, h,
                                    (hipStream_t)stream, sk, sk_bytes);
}
#endif  // WISE_DEBUG_KNOBS

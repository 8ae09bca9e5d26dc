// HP-2: IndexSQ8bit — exhaustive inner-product search over rows kept as ONE byte per dimension (faiss IndexScalarQuantizer(d,
// QT_8bit, METRIC_INNER_PRODUCT) with RS_minmax under an IndexIDMap).  The index is codes [N, d] uint8 plus trained [2 d] fp32
// (vmin, then vdiff: wise_sq_train / wise_sq_minmax) and the ids: d bytes a row, no fp32 rows, no shadow.
//   wise_ipsq8_topk           THE EXACT SCAN: score(q, r) = q0[q] + s_0 of the wise_ivfsq_scan contract (Codec8 and sq_score_loads
//                             of sq_codec.h, the device code IndexIVFSQ8 scores with); top-k per query
//   wise_ipsq8_topk_pos       the same over an ascending list of positions (an IDSelector resolved by ivf_select.hip)
//   wise_ipsq8_range_*        count / fill of range_search (range_common.h) over the same score
//   wise_ipsq8_reconstruct    reconstruct_batch: faiss's Codec8bit decode of the row that carries an id
//   wise_ipsq8_prepare        norms[0] = the largest norm of a row's codes taken as the numbers 0 .. 255
//   wise_ipsq8_topk_batched   3 or more queries: threshold, collect on v_mfma_f32_32x32x16_f16 over codes expanded in registers, exact
//                             re-scoring — the bits of wise_ipsq8_topk by construction
// Every entry point takes the queries themselves and `trained`: W and q0 are wise_sq_query's, written into the head of the call's
// workspace (QuerySlots).  The scans, the range pair and the batched search are flat_codec_scan.h's under the policy MetricIP8 below.
#include "flat_codec_scan.h"

namespace wise {
namespace ipsq8 {

using namespace flat_codec;

// the head of every workspace: W [nq, d] and q0 [nq] of wise_sq_query; what the shared drivers use follows
struct QuerySlots {
    float* W;
    float* q0;
    unsigned char* rest;
    static size_t bytes(int nq, int d) { return align_up((size_t)nq * d * sizeof(float), 256) + align_up((size_t)nq * sizeof(float), 256); }
    QuerySlots(void* workspace, int nq, int d) {
        unsigned char* b = reinterpret_cast<unsigned char*>(workspace);
        W = reinterpret_cast<float*>(b);
        q0 = reinterpret_cast<float*>(b + align_up((size_t)nq * d * sizeof(float), 256));
        rest = b + bytes(nq, d);
    }
};

// wise_ipsq8_reconstruct: sq16_reconstruct_kernel (ip_sq16.hip) for this payload; the decode is decode_kernel's (ivf_sq.hip) without a
// centroid: vmin + ((code + 0.5) / 255) * vdiff, each operation rounded to fp32 on its own.  The highest position wins where an id repeats
__global__ __launch_bounds__(256) void sq8_reconstruct_kernel(const unsigned char* __restrict__ codes, const float* __restrict__ trained,
                                                              long long N, int d, const long long* __restrict__ ids, long long id_base,
                                                              const long long* __restrict__ qids, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int i = blockIdx.x;
    const long long row = row_of_id(ids, id_base, N, qids[i]);
    for (int c = threadIdx.x; c < d; c += blockDim.x) {
        float y = __builtin_nanf("");
        if (row >= 0) {
            const float xi = ((float)codes[(size_t)row * d + c] + 0.5f) / 255.0f;
            const float s = xi * trained[d + c];
            y = trained[c] + s;
        }
        out[(size_t)i * d + c] = y;
    }
}

// wise_ipsq8_prepare: one wave per row at a time; lane l sums the squares of the 16 codes of piece l (d <= 1024: at most 64 pieces)
// as integers — 255^2 * 1024 < 2^32, so the sum is exact and its order does not matter — and the maximum over the rows is exact too.
// norms[0] holds the integer while the rows are reduced; the finish kernel makes sqrtf((float)max) of it.
__global__ __launch_bounds__(256) void sq8_norm_kernel(const unsigned char* __restrict__ codes, long long N, int d,
                                                       unsigned* __restrict__ cell) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pieces = d >> 4;
    unsigned best = 0u;
    for (long long r = (long long)blockIdx.x * 4 + wave; r < N; r += (long long)gridDim.x * 4) {
        unsigned s = 0u;
        if (lane < pieces) {
            const u32x4 x = reinterpret_cast<const u32x4*>(codes + (size_t)r * d)[lane];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const unsigned v = (x[j] >> (8 * b)) & 0xffu;
                    s += v * v;
                }
        }
        for (int o = 32; o >= 1; o >>= 1) s += (unsigned)__shfl_xor((int)s, o, 64);
        best = s > best ? s : best;
    }
    if (lane == 0) atomicMax(cell, best);
}
__global__ void sq8_norm_finish_kernel(float* __restrict__ norms) {
    if (threadIdx.x == 0 && blockIdx.x == 0) norms[0] = sqrtf((float)*reinterpret_cast<const unsigned*>(norms));
}

// ---- the batched search (wise_ipsq8_topk_batched): the pass of flat_codec_scan.h.  What is this type's own:
//   stage    Q is the pass's rows of W.  Per query a power of two 2^e that puts the largest |W| into [2^14, 2^15) — 23 % of the weights
//            of a d = 128 study set and 98 % at d = 1024 are below binary16's normal range as they are, none of any size once scaled;
//            ldexpf is exact — then the image f16(2^e W) and, IN THE SCALED SPACE, eps = the bound on |MFMA sum - 2^e s_0| of any row
//            (DESIGN.md section 4): |2^e W - f16(2^e W)| norms[0] (Cauchy-Schwarz on the image's rounding; a code 0 .. 255 is a
//            binary16 value, so there is no row-side term) + d 2^-22 |2^e W| norms[0] (fp32 accumulation of both sums).  A query whose
//            weights or q0 are not finite, whose largest weight is below 2^-112 (e > 126: 2^e s_0 would magnify what the exact
//            chain lost below the normal range) or whose band is not finite hands the pass to the exact scan at once
//   sample   t = the k-th score over the sample is a lower bound of the index's exact k-th: a row r of the exact top-k has
//            fl(q0 + s_0(r)) >= t, so s_0(r) >= (t - q0) - 2^-23 |t| (the final addition's rounding), and its MFMA sum is at least
//            thr = 2^e ((t - q0) - slack) - eps
//   collect  every (query, row) with MFMA sum >= thr[query] is listed
// block = one wave = one query
__global__ __launch_bounds__(64) void sq8_stage_kernel(const float* __restrict__ W, int d, const float* __restrict__ norms, BatchSlots ws) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, q = blockIdx.x;
    float mx = 0.f;
    bool bad = false;
    for (int i = lane; i < d; i += 64) {
        const float a = fabsf(W[(size_t)q * d + i]);
        bad = bad || !is_finite_f32(a);
        mx = a > mx ? a : mx;
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const float other = __shfl_xor(mx, o, 64);
        mx = other > mx ? other : mx;
    }
    bad = __ballot(bad) != 0;
    // e = 14 - floor(log2 mx) from the bits of mx; a subnormal or zero exponent field: no scaling for all-zero weights, else e > 126
    int e = 0;
    bool unscalable = false;
    if (!bad && mx > 0.f) {
        const int ex = (int)((__float_as_uint(mx) >> 23) & 0xffu) - 127;
        e = 14 - ex;
        if (ex == -127 || e > 126) { unscalable = true; e = 0; }
    }
    float e2 = 0.f, w2 = 0.f;
    for (int i = lane; i < d; i += 64) {
        const float v = ldexpf(W[(size_t)q * d + i], e);
        const _Float16 h = (_Float16)v;
        ws.q16[(size_t)q * d + i] = h;
        const float back = (float)h, r = v - back;
        bad = bad || !is_finite_f32(back);
        e2 = fmaf(r, r, e2);
        w2 = fmaf(v, v, w2);
    }
    e2 = wave_sum(e2);
    w2 = wave_sum(w2);
    bad = __ballot(bad) != 0;
    if (lane == 0) {
        const float M = norms[0];
        // every factor rounded up a little: the sums above and M are themselves fp32 results (relative error < d 2^-23)
        float eps = (sqrtf(e2) * 1.001f + (float)d * 2.384185791015625e-07f * sqrtf(w2) * 1.001f) * M * 1.001f;
        if (bad || unscalable || !is_finite_f32(eps) || !is_finite_f32(ws.base[q])) {
            eps = __builtin_inff();
            *ws.flag = 1;                                         // (every block that raises it stores the same value)
        }
        ws.eps[q] = eps;
        ws.qexp[q] = e;
        ws.thr[q] = -__builtin_inff();
        ws.ctl[q] = 0;
    }
}

// thr of a query whose k-th best exact score over some of the rows is t, in the scaled space of its image, rounded down.  u = 2^-24:
// the final addition loses at most 2 u |t|, t - q0 and the subtraction of the slack at most u (|t| + |q0|) each: 2^-21 (|t| + |q0|)
// is twice their sum.  ldexpf is exact unless it leaves the normal range: below it the 1e-37 pays, above it the threshold stays open.
__device__ __forceinline__ float threshold_below_scaled(float t, float q0, int e, float eps) {
#pragma clang fp contract(off)
    const float s = (t - q0) - (fabsf(t) + fabsf(q0)) * 4.76837158203125e-07f;
    const float v = ldexpf(s, e);
    return (v - eps * 1.0001f) - fabsf(v) * 4.76837158203125e-07f - 1e-37f;
}

// codes b0 .. b3 of a word -> the binary16 pairs (b0, b1) and (b2, b3): v_perm_b32 puts each code under the exponent byte 0x64 —
// 0x6400 | b is 1024 + b exactly, the ulp of binary16 in [1024, 2048) being 1 — and the operand is that minus 1024 (packed binary16
// subtractions, exact).  Selector bytes 0 .. 3 pick from the word, 4 from the pattern.
__device__ __forceinline__ unsigned codes_lo(unsigned word) { return __builtin_amdgcn_perm(0x64646464u, word, 0x04010400u); }
__device__ __forceinline__ unsigned codes_hi(unsigned word) { return __builtin_amdgcn_perm(0x64646464u, word, 0x04030402u); }

// THE POLICY (flat_codec_scan.h): the score is q0 + s, larger is better
struct MetricIP8 {
    using Codec = Codec8;
    static constexpr float PAD = -3.4028234663852886e38f;
    static constexpr bool FLIP = false;
    static __device__ __forceinline__ float base(const float* __restrict__ q0, int q) { return q0[q]; }
    static __device__ __forceinline__ float score(float s, float b) {
#pragma clang fp contract(off)
        return b + s;
    }
    static __device__ __forceinline__ float key_score(float sc) { return sc; }
    static __device__ __forceinline__ float out_score(float ks) { return ks; }
    static __device__ __forceinline__ bool range_hit(float sc, float radius) { return sc > radius; }
    static __device__ __forceinline__ float thr_open() { return -__builtin_inff(); }
    static __device__ __forceinline__ float thr_shut() { return 3.4028234663852886e38f; }
    static __device__ __forceinline__ float tighten(float thr, float t, const BatchSlots& ws, int q) {
        t = threshold_below_scaled(t, ws.base[q], ws.qexp[q], ws.eps[q]);
        return is_finite_f32(t) && t > thr ? t : thr;
    }
    using Piece = f16x8;
    static __device__ __forceinline__ f32x16 mfma(Piece a, Piece b, f32x16 acc) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
    }
    static constexpr int LOAD_PIECES = 2;
    static __device__ __forceinline__ Piece operand(u32x4 x, int p) {
        const unsigned a = x[2 * p], b = x[2 * p + 1];
        const u32x4 o = {codes_lo(a), codes_hi(a), codes_lo(b), codes_hi(b)};
        const _Float16 k = (_Float16)1024.0f;
        const f16x8 bias = {k, k, k, k, k, k, k, k};
        return __builtin_bit_cast(f16x8, o) - bias;
    }
    static constexpr bool QUERY_EXP = true;
    static constexpr bool HALF_NORMS = false;
    static __device__ __forceinline__ bool candidate(float, float acc, float thr) { return !(acc < thr); }
    static const char* stage(const float* W, int d, const float* norms, const BatchSlots& ws, int nq, hipStream_t st) {
        hipLaunchKernelGGL(sq8_stage_kernel, dim3(nq), dim3(64), 0, st, W, d, norms, ws);
        return "sq8_stage_kernel";
    }
};

// the arguments every entry point shares beyond the shared drivers' checks
static int sq8_args(const char* what, const float* trained, const void* workspace) {
    WISE_CHECK_ARG(trained, "%s: null pointer (trained)", what);
    WISE_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "%s: the workspace must be 16-byte aligned", what);
    return WISE_OK;
}

static int sq8_topk(const char* what, const uint8_t* codes, const float* trained, int64_t N, int d, bool by_pos, const int64_t* pos,
                    int64_t n_pos, const float* Q, int nq, int k, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI,
                    void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = topk_args(what, codes, N, d, Q, nq, k, outD, outI)) return rc;
    if (by_pos)
        WISE_CHECK_ARG(n_pos >= 0 && n_pos <= N && (pos || n_pos == 0), "%s: n_pos=%lld out of [0, N=%lld] or null positions", what,
                       (long long)n_pos, (long long)N);
    const int64_t n = by_pos ? n_pos : N;
    const size_t need = wise_ipsq8_topk_workspace_bytes(n, d, nq, k);
    WISE_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace %zu < %zu bytes", what, workspace_bytes, need);
    if (int rc = sq8_args(what, trained, workspace)) return rc;
    const QuerySlots qs(workspace, nq, d);
    if (int rc = wise_sq_query(Q, trained, nq, d, qs.W, qs.q0, stream)) return rc;
    return flat_topk<MetricIP8>(codes, n, d, qs.W, qs.q0, nq, k, ids, id_base, outD, outI, qs.rest, (hipStream_t)stream,
                                by_pos && n_pos > 0 ? reinterpret_cast<const long long*>(pos) : nullptr, nullptr);
}

}  // namespace ipsq8
}  // namespace wise

using namespace wise;
using namespace wise::ipsq8;

extern "C" size_t wise_ipsq8_topk_workspace_bytes(int64_t N, int d, int nq, int k) {
    const size_t scan = topk_workspace_bytes(N, d, nq, k);
    return scan ? QuerySlots::bytes(nq, d) + scan : 0;
}

extern "C" int wise_ipsq8_topk(const uint8_t* codes, const float* trained, int64_t N, int d, const float* Q, int nq, int k,
                               const int64_t* ids, int64_t id_base, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes,
                               void* stream) {
    return sq8_topk("ipsq8_topk", codes, trained, N, d, false, nullptr, 0, Q, nq, k, ids, id_base, outD, outI, workspace, workspace_bytes,
                    stream);
}

extern "C" int wise_ipsq8_topk_pos(const uint8_t* codes, const float* trained, int64_t N, int d, const int64_t* pos, int64_t n_pos,
                                   const float* Q, int nq, int k, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    return sq8_topk("ipsq8_topk_pos", codes, trained, N, d, true, pos, n_pos, Q, nq, k, ids, id_base, outD, outI, workspace,
                    workspace_bytes, stream);
}

// the range pair: the count pass writes W and q0 into the head of the workspace, the fill pass (same workspace, same queries) reads them
extern "C" size_t wise_ipsq8_range_workspace_bytes(int64_t N, int d, int nq) {
    const size_t scan = range_workspace(N, d, nq);
    return range_shape_ok(N, d, nq) ? QuerySlots::bytes(nq, d) + scan : 0;
}

extern "C" int wise_ipsq8_range_count(const uint8_t* codes, const float* trained, int64_t N, int d, const float* Q, int nq, float radius,
                                      const uint32_t* keep, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    WISE_CHECK_ARG(range_shape_ok(N, d, nq), "ipsq8_range_count: N=%lld d=%d nq=%d out of range (d %% 16 == 0 in [16, 1024], nq <= 65535)",
                   (long long)N, d, nq);
    const size_t head = QuerySlots::bytes(nq, d);
    WISE_CHECK_ARG(workspace && workspace_bytes >= head + range_workspace(N, d, nq), "ipsq8_range_count: workspace %zu < %zu bytes",
                   workspace_bytes, head + range_workspace(N, d, nq));
    if (int rc = sq8_args("ipsq8_range_count", trained, workspace)) return rc;
    const QuerySlots qs(workspace, nq, d);
    if (int rc = range_args("ipsq8_range_count", codes, N, d, Q, nq, radius, qs.rest, workspace_bytes - head)) return rc;
    WISE_CHECK_ARG(counts, "ipsq8_range_count: null pointer");
    if (int rc = wise_sq_query(Q, trained, nq, d, qs.W, qs.q0, stream)) return rc;
    return range_count<MetricIP8>("ipsq8_range_count", codes, N, d, qs.W, qs.q0, nq, radius, keep, counts, qs.rest, workspace_bytes - head,
                                  stream);
}

extern "C" int wise_ipsq8_range_fill(const uint8_t* codes, const float* trained, int64_t N, int d, const float* Q, int nq, float radius,
                                     const int64_t* ids, int64_t id_base, const int64_t* lims, float* outD, int64_t* outI, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    WISE_CHECK_ARG(range_shape_ok(N, d, nq), "ipsq8_range_fill: N=%lld d=%d nq=%d out of range (d %% 16 == 0 in [16, 1024], nq <= 65535)",
                   (long long)N, d, nq);
    const size_t head = QuerySlots::bytes(nq, d);
    WISE_CHECK_ARG(workspace && workspace_bytes >= head + range_workspace(N, d, nq), "ipsq8_range_fill: workspace %zu < %zu bytes",
                   workspace_bytes, head + range_workspace(N, d, nq));
    if (int rc = sq8_args("ipsq8_range_fill", trained, workspace)) return rc;
    const QuerySlots qs(workspace, nq, d);
    if (int rc = range_args("ipsq8_range_fill", codes, N, d, Q, nq, radius, qs.rest, workspace_bytes - head)) return rc;
    WISE_CHECK_ARG(lims && outD && outI, "ipsq8_range_fill: null pointer");
    return range_fill<MetricIP8>("ipsq8_range_fill", codes, N, d, qs.W, qs.q0, nq, radius, ids, id_base, lims, outD, outI, qs.rest,
                                 workspace_bytes - head, stream);
}

// search_grouped, stage 1: ord [nq][N] = the ordered image of q0 + s_0 of every (query, row), 0 for the rows keep clears.  W and q0
// are wise_sq_query's for the queries, as the wise_ivfsq_* entry points take them: no workspace
extern "C" int wise_ipsq8_group_scores(const uint8_t* codes, int64_t N, int d, const float* W, const float* q0, int nq, const uint32_t* keep,
                                       uint32_t* ord, void* stream) {
    WISE_CHECK_ARG(q0, "ipsq8_group_scores: null pointer (q0)");
    return group_scores<MetricIP8>("ipsq8_group_scores", codes, N, d, W, q0, nq, keep, ord, stream);
}

extern "C" int wise_ipsq8_reconstruct(const uint8_t* codes, const float* trained, int64_t N, int d, const int64_t* ids, int64_t id_base,
                                      const int64_t* query_ids, int n, float* out, void* stream) {
    WISE_CHECK_ARG(shape_ok(d), "ipsq8_reconstruct: d=%d unsupported (d %% 16 == 0 in [16, 1024])", d);
    WISE_CHECK_ARG(N >= 0 && n >= 0 && trained && (codes || N == 0) && (n == 0 || (query_ids && out)), "ipsq8_reconstruct: bad argument");
    if (n == 0) return WISE_OK;
    hipLaunchKernelGGL(sq8_reconstruct_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, codes, trained, (long long)N, d,
                       reinterpret_cast<const long long*>(ids), (long long)id_base, reinterpret_cast<const long long*>(query_ids), out);
    WISE_LAUNCH_CHECK("sq8_reconstruct_kernel");
    return WISE_OK;
}

extern "C" int wise_ipsq8_prepare(const uint8_t* codes, int64_t N, int d, float* norms, void* stream) {
    WISE_CHECK_ARG(shape_ok(d), "ipsq8_prepare: d=%d unsupported (d %% 16 == 0 in [16, 1024])", d);
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll && norms && (codes || N == 0), "ipsq8_prepare: bad argument");
    WISE_CHECK_ARG(((uintptr_t)codes & 15) == 0, "ipsq8_prepare: codes must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(norms, 0, sizeof(float), st);
    if (e != hipSuccess) { set_error("ipsq8_prepare: memset: %s", hipGetErrorString(e)); return (int)e; }
    if (N == 0) return WISE_OK;
    hipLaunchKernelGGL(sq8_norm_kernel, dim3(wave_row_grid(N)), dim3(256), 0, st, codes, (long long)N, d, reinterpret_cast<unsigned*>(norms));
    WISE_LAUNCH_CHECK("sq8_norm_kernel");
    hipLaunchKernelGGL(sq8_norm_finish_kernel, dim3(1), dim3(64), 0, st, norms);
    WISE_LAUNCH_CHECK("sq8_norm_finish_kernel");
    return WISE_OK;
}

extern "C" size_t wise_ipsq8_topk_batched_workspace_bytes(int64_t N, int d, int nq, int k) {
    const size_t pass = batched_workspace_bytes<MetricIP8>(N, d, nq, k);
    return pass ? QuerySlots::bytes(nq, d) + pass : 0;
}

extern "C" int wise_ipsq8_topk_batched(const uint8_t* codes, const float* trained, const float* norms, int64_t N, int d, const float* Q,
                                       int nq, int k, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI, int32_t* counters,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = batched_args("ipsq8_topk_batched", codes, N, d, Q, nq, k, outD, outI, norms, workspace, workspace_bytes,
                              wise_ipsq8_topk_batched_workspace_bytes(N, d, nq, k)))
        return rc;
    if (int rc = sq8_args("ipsq8_topk_batched", trained, workspace)) return rc;
    const QuerySlots qs(workspace, nq, d);
    if (int rc = wise_sq_query(Q, trained, nq, d, qs.W, qs.q0, stream)) return rc;
    return topk_batched<MetricIP8>("ipsq8_topk_batched", codes, codes, nullptr, norms, N, d, qs.W, qs.q0, nq, k, ids, id_base, outD, outI,
                                   counters, qs.rest, (hipStream_t)stream);
}

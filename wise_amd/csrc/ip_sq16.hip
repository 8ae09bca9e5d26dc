// HP-2: IndexSQfp16 — exhaustive inner-product search over rows stored as IEEE binary16 (faiss IndexScalarQuantizer(d, QT_fp16,
// METRIC_INNER_PRODUCT) under an IndexIDMap).  The index is ONE [N, d] array of halves, 2 d bytes a row: no fp32 rows, no shadow.
//   wise_ipsq16_topk           THE EXACT SCAN: score(q, r) = s_0 of the wise_ivfsq16_scan contract (Codec16 and sq_score_loads of
//                              sq_codec.h, the device code IndexIVFSQfp16 scores with), no bias; top-k per query
//   wise_ipsq16_topk_pos       the same over an ascending list of positions (an IDSelector resolved by ivf_select.hip)
//   wise_ipsq16_range_*        count / fill of range_search (range_common.h) over the same score
//   wise_ipsq16_reconstruct    reconstruct_batch: the widened halves of the row that carries an id
//   wise_ipsq16_prepare        norms[0] = the largest row norm, what the batched search's error band needs
//   wise_ipsq16_topk_batched   3 or more queries: threshold, collect on v_mfma_f32_32x32x16_f16, exact re-scoring — the bits of
//                              wise_ipsq16_topk by construction
// The scans, the range pair and the batched search are flat_codec_scan.h's under the policy MetricIP16 below (how a wave-load is
// laid out: there).  Here: the policy, the kernels that belong to this type alone and the entry points.
#include "flat_codec_scan.h"

namespace wise {
namespace ipsq16 {

using namespace flat_codec;

// wise_ipsq16_reconstruct: reconstruct_kernel (ip_topk.hip) for this payload
__global__ __launch_bounds__(256) void sq16_reconstruct_kernel(const _Float16* __restrict__ rows, long long N, int d,
                                                               const long long* __restrict__ ids, long long id_base,
                                                               const long long* __restrict__ qids, float* __restrict__ out) {
    const int i = blockIdx.x;
    const long long row = row_of_id(ids, id_base, N, qids[i]);
    for (int c = threadIdx.x; c < d; c += blockDim.x)
        out[(size_t)i * d + c] = row >= 0 ? (float)rows[(size_t)row * d + c] : __builtin_nanf("");
}

// wise_ipsq16_prepare: one wave per row at a time; the norm is sqrtf of half_row_square_sum (flat_codec_scan.h): a row's norm depends
// on the row alone.  The maximum is exact, and non-negative floats order as their bit patterns: atomicMax on the bits gives the same
// value in any order.
__global__ __launch_bounds__(256) void sq16_norm_kernel(const unsigned char* __restrict__ rows, long long N, int d,
                                                        unsigned* __restrict__ norm_bits) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float best = 0.f;
    for (long long r = (long long)blockIdx.x * 4 + wave; r < N; r += (long long)gridDim.x * 4) {
        const float s = sqrtf(half_row_square_sum(rows, r, d, lane));
        best = s > best ? s : best;                              // (a NaN norm is never kept: non-finite rows are outside the contract)
    }
    if (lane == 0) atomicMax(norm_bits, __float_as_uint(best));
}

// ---- the batched search (wise_ipsq16_topk_batched): the pass of flat_codec_scan.h.  What is this type's own:
//   stage    the queries rounded to binary16 (ONE piece; a query that does not fit binary16's range hands the pass to the exact
//            scan at once) and, per query, eps = the bound on |MFMA score - exact-scan score| of any
//            row: |q - f16(q)| norms[0] (Cauchy-Schwarz on the query's rounding; the rows are used as stored,
//            so there is no row-side term) + d 2^-22 |q| norms[0] (fp32 accumulation of both sums)
//   sample   t = the k-th score over the sample is a lower bound of the index's exact k-th, so every row of the exact top-k has an
//            MFMA score >= thr = t - eps
//   collect  every (query, row) with MFMA score >= thr[query] is listed
// block = one wave = one query
__global__ __launch_bounds__(64) void sq16_stage_kernel(const float* __restrict__ Q, int d, const float* __restrict__ norms,
                                                        BatchSlots ws) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, q = blockIdx.x;
    float e2 = 0.f, q2 = 0.f;
    bool bad = false;
    for (int i = lane; i < d; i += 64) {
        const float v = Q[(size_t)q * d + i];
        const _Float16 h = (_Float16)v;
        ws.q16[(size_t)q * d + i] = h;
        const float back = (float)h, r = v - back;
        bad = bad || !is_finite_f32(back);                        // the half is infinite or NaN
        e2 = fmaf(r, r, e2);
        q2 = fmaf(v, v, q2);
    }
    e2 = wave_sum(e2);
    q2 = wave_sum(q2);
    const bool any_bad = __ballot(bad) != 0;
    if (lane == 0) {
        const float M = norms[0];
        // every factor rounded up a little: the sums above and M are themselves fp32 results (relative error < d 2^-23)
        float eps = (sqrtf(e2) * 1.001f + (float)d * 2.384185791015625e-07f * sqrtf(q2) * 1.001f) * M * 1.001f;
        // (by its bits: under the default fp contraction `eps - eps` fuses with the product above into its rounding error)
        // A query whose binary16 image is not finite (a component beyond 65504), or whose band is not, has no usable matrix-core
        // score (inf * 0 and inf - inf are NaN): it raises the pass's flag here — the host cleared it before this launch — and the
        // exact scan answers the pass.  Every block that raises it stores the same value.
        if (any_bad || !is_finite_f32(eps)) {
            eps = __builtin_inff();
            *ws.flag = 1;
        }
        ws.eps[q] = eps;
        ws.thr[q] = -__builtin_inff();
        ws.ctl[q] = 0;
    }
}

// thr of a query whose k-th best exact score over some of the rows is t: t - eps, rounded down
__device__ __forceinline__ float threshold_below(float t, float eps) {
#pragma clang fp contract(off)
    return (t - eps * 1.0001f) - fabsf(t) * 4.76837158203125e-07f - 1e-37f;
}

// THE POLICY (flat_codec_scan.h): the score is the inner product itself, larger is better
struct MetricIP16 : PlainPolicy {
    using Codec = Codec16;
    static constexpr float PAD = -3.4028234663852886e38f;
    static constexpr bool FLIP = false;
    static __device__ __forceinline__ float key_score(float s) { return s; }
    static __device__ __forceinline__ float out_score(float ks) { return ks; }
    static __device__ __forceinline__ bool range_hit(float s, float radius) { return s > radius; }
    static __device__ __forceinline__ float thr_open() { return -__builtin_inff(); }
    static __device__ __forceinline__ float thr_shut() { return 3.4028234663852886e38f; }
    static __device__ __forceinline__ float tighten(float thr, float t, const BatchSlots& ws, int q) {
        t = threshold_below(t, ws.eps[q]);
        return t > thr ? t : thr;
    }
    using Piece = f16x8;
    static __device__ __forceinline__ f32x16 mfma(Piece a, Piece b, f32x16 acc) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
    }
    static constexpr bool HALF_NORMS = false;
    static __device__ __forceinline__ bool candidate(float, float acc, float thr) { return !(acc < thr); }
    static const char* stage(const float* Q, int d, const float* norms, const BatchSlots& ws, int nq, hipStream_t st) {
        hipLaunchKernelGGL(sq16_stage_kernel, dim3(nq), dim3(64), 0, st, Q, d, norms, ws);
        return "sq16_stage_kernel";
    }
};

}  // namespace ipsq16
}  // namespace wise

using namespace wise;
using namespace wise::ipsq16;

extern "C" size_t wise_ipsqfp16_topk_workspace_bytes(int64_t N, int d, int nq, int k) { return topk_workspace_bytes(N, d, nq, k); }

extern "C" int wise_ipsq16_topk(const uint16_t* rows, int64_t N, int d, const float* Q, int nq, int k, const int64_t* ids,
                                int64_t id_base, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream) {
    return topk_entry<MetricIP16>("ipsq16_topk", rows, N, d, false, nullptr, 0, Q, nullptr, nq, k, ids, id_base, outD, outI, workspace,
                                  workspace_bytes, stream);
}

extern "C" int wise_ipsq16_topk_pos(const uint16_t* rows, int64_t N, int d, const int64_t* pos, int64_t n_pos, const float* Q, int nq,
                                    int k, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    return topk_entry<MetricIP16>("ipsq16_topk_pos", rows, N, d, true, pos, n_pos, Q, nullptr, nq, k, ids, id_base, outD, outI, workspace,
                                  workspace_bytes, stream);
}

extern "C" size_t wise_ipsqfp16_range_workspace_bytes(int64_t N, int d, int nq) { return range_workspace(N, d, nq); }

extern "C" int wise_ipsq16_range_count(const uint16_t* rows, int64_t N, int d, const float* Q, int nq, float radius, const uint32_t* keep,
                                       int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    return range_count<MetricIP16>("ipsq16_range_count", rows, N, d, Q, nullptr, nq, radius, keep, counts, workspace, workspace_bytes, stream);
}

extern "C" int wise_ipsq16_range_fill(const uint16_t* rows, int64_t N, int d, const float* Q, int nq, float radius, const int64_t* ids,
                                      int64_t id_base, const int64_t* lims, float* outD, int64_t* outI, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    return range_fill<MetricIP16>("ipsq16_range_fill", rows, N, d, Q, nullptr, nq, radius, ids, id_base, lims, outD, outI, workspace,
                                  workspace_bytes, stream);
}

// search_grouped, stage 1: ord [nq][N] = the ordered key score of every (query, row), 0 for the rows keep clears
extern "C" int wise_ipsq16_group_scores(const uint16_t* rows, int64_t N, int d, const float* Q, int nq, const uint32_t* keep, uint32_t* ord,
                                        void* stream) {
    return group_scores<MetricIP16>("ipsq16_group_scores", rows, N, d, Q, nullptr, nq, keep, ord, stream);
}

extern "C" int wise_ipsq16_reconstruct(const uint16_t* rows, int64_t N, int d, const int64_t* ids, int64_t id_base, const int64_t* query_ids,
                                       int n, float* out, void* stream) {
    WISE_CHECK_ARG(shape_ok(d), "ipsq16_reconstruct: d=%d unsupported (d %% 16 == 0 in [16, 1024])", d);
    WISE_CHECK_ARG(N >= 0 && n >= 0 && (rows || N == 0) && (n == 0 || (query_ids && out)), "ipsq16_reconstruct: bad argument");
    if (n == 0) return WISE_OK;
    hipLaunchKernelGGL(sq16_reconstruct_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const _Float16*>(rows),
                       (long long)N, d, reinterpret_cast<const long long*>(ids), (long long)id_base,
                       reinterpret_cast<const long long*>(query_ids), out);
    WISE_LAUNCH_CHECK("sq16_reconstruct_kernel");
    return WISE_OK;
}

extern "C" int wise_ipsq16_prepare(const uint16_t* rows, int64_t N, int d, float* norms, void* stream) {
    WISE_CHECK_ARG(shape_ok(d), "ipsq16_prepare: d=%d unsupported (d %% 16 == 0 in [16, 1024])", d);
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll && norms && (rows || N == 0), "ipsq16_prepare: bad argument");
    WISE_CHECK_ARG(((uintptr_t)rows & 15) == 0, "ipsq16_prepare: rows must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(norms, 0, sizeof(float), st);
    if (e != hipSuccess) { set_error("ipsq16_prepare: memset: %s", hipGetErrorString(e)); return (int)e; }
    if (N == 0) return WISE_OK;
    hipLaunchKernelGGL(sq16_norm_kernel, dim3(wave_row_grid(N)), dim3(256), 0, st, reinterpret_cast<const unsigned char*>(rows), (long long)N,
                       d, reinterpret_cast<unsigned*>(norms));
    WISE_LAUNCH_CHECK("sq16_norm_kernel");
    return WISE_OK;
}

extern "C" size_t wise_ipsqfp16_topk_batched_workspace_bytes(int64_t N, int d, int nq, int k) {
    return batched_workspace_bytes<MetricIP16>(N, d, nq, k);
}

extern "C" int wise_ipsq16_topk_batched(const uint16_t* rows, const float* norms, int64_t N, int d, const float* Q, int nq, int k,
                                        const int64_t* ids, int64_t id_base, float* outD, int64_t* outI, int32_t* counters,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = batched_args("ipsq16_topk_batched", rows, N, d, Q, nq, k, outD, outI, norms, workspace, workspace_bytes,
                              wise_ipsqfp16_topk_batched_workspace_bytes(N, d, nq, k)))
        return rc;
    return topk_batched<MetricIP16>("ipsq16_topk_batched", rows, rows, nullptr, norms, N, d, Q, nullptr, nq, k, ids, id_base, outD, outI, counters,
                                    workspace, (hipStream_t)stream);
}

// HP-2: IndexSQfp16L2 — exhaustive squared-L2 search over rows stored as IEEE binary16 (faiss IndexScalarQuantizer(d, QT_fp16,
// METRIC_L2) under an IndexIDMap).  The index is the ONE [N, d] array of halves IndexSQfp16 keeps, 2 d bytes a row: no fp32 rows
// and no second copy of the rows.
//   wise_l2sq16_topk           THE EXACT SCAN: dist(q, r) = s_0 of Codec16L2 under sq_score_loads (sq_codec.h); the k smallest per query
//   wise_l2sq16_topk_pos       the same over an ascending list of positions (an IDSelector resolved by ivf_select.hip)
//   wise_l2sq16_range_*        count / fill of range_search (range_common.h) over the same distance: a hit iff dist < radius
//   wise_l2sq16_prepare        half[r] = |h_r|^2 / 2 and norms[0] = the largest row norm: all the batched search keeps beside the rows
//   wise_l2sq16_topk_batched   3 or more queries: threshold, collect on v_mfma_f32_32x32x16_f16 over the stored rows as loaded, exact
//                              re-scoring — the bits of wise_l2sq16_topk by construction
// The score is the negated distance, as in l2_topk.hip: keys, ties, the per-wave lists and merge_keys_kernel run unchanged and the
// sign flips back behind the merge (l2_flip_launch).  The scans, the range pair and the batched search are flat_codec_scan.h's under
// the policy MetricL2SQ16 below.  Here: the policy, the kernels that belong to this type alone and the entry points.
#include "flat_codec_scan.h"

namespace wise {
namespace l2sq16 {

using namespace flat_codec;

// wise_l2sq16_prepare, first launch: half[r] = 0.5f * |h_r|^2.  One wave per row at a time; the sum is half_row_square_sum's
// (flat_codec_scan.h), halved (exact): a row's half-norm depends on the row alone.
__global__ __launch_bounds__(256) void l2sq16_half_norm_kernel(const unsigned char* __restrict__ rows, long long N, int d,
                                                               float* __restrict__ half) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long r = (long long)blockIdx.x * 4 + wave; r < N; r += (long long)gridDim.x * 4) {
        const float s = half_row_square_sum(rows, r, d, lane);
        if (lane == 0) half[r] = 0.5f * s;
    }
}

// wise_l2sq16_prepare, second launch: ONE block folds the N half-norms into norms[0] = sqrtf(2 max_r half[r]) — the largest row
// norm.  A maximum is exact in any order, so no atomic is needed and the same rows give the same bits; the block reads N 4 bytes
// once per change of the rows, which no search waits for twice.
__global__ __launch_bounds__(1024) void l2sq16_max_norm_kernel(const float* __restrict__ half, long long N, float* __restrict__ norms) {
    __shared__ float part[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float best = 0.f;                                             // (a NaN is never kept: non-finite rows are outside the contract)
    for (long long i0 = threadIdx.x; i0 < N; i0 += 4 * 1024) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long i = i0 + (long long)j * 1024;
            v[j] = i < N ? half[i] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) best = v[j] > best ? v[j] : best;
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const float v = __shfl_xor(best, o, 64);
        best = v > best ? v : best;
    }
    if (lane == 0) part[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) best = part[w] > best ? part[w] : best;
        norms[0] = sqrtf(2.f * best);
    }
}

// ---- the batched search (wise_l2sq16_topk_batched): wise_l2_topk_batched's pass over rows that ARE their own matrix-core operands:
// l2_stage_kernel<_Float16, false> and threshold_above of flat_codec_scan.h — the binary16 image of the queries, and eps without the
// rows' rounding term (M = norms[0] = max |h|).

// THE POLICY (flat_codec_scan.h): the keys order the negated distance; the collect operand is the stored row
struct MetricL2SQ16 : PlainPolicy {
    using Codec = Codec16L2;
    static constexpr float PAD = 3.4028234663852886e38f;
    static constexpr bool FLIP = true;
    static int flip(float* D, int n, const int* gate, hipStream_t st) { return l2_flip_launch(D, n, gate, st); }
    static __device__ __forceinline__ float key_score(float s) { return -s; }
    static __device__ __forceinline__ float out_score(float ks) { return -ks; }
    static __device__ __forceinline__ bool range_hit(float s, float radius) { return s < radius; }
    static __device__ __forceinline__ float thr_open() { return __builtin_inff(); }
    static __device__ __forceinline__ float thr_shut() { return -__builtin_inff(); }
    static __device__ __forceinline__ float tighten(float thr, float t, const BatchSlots& ws, int q) {
        t = threshold_above(t, ws.q2[q], ws.eps[q]);
        return t < thr ? t : thr;
    }
    using Piece = f16x8;
    static __device__ __forceinline__ f32x16 mfma(Piece a, Piece b, f32x16 acc) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
    }
    static constexpr bool HALF_NORMS = true;
    static __device__ __forceinline__ bool candidate(float hv, float acc, float thr) { return !(hv - acc > thr); }
    static const char* stage(const float* Q, int d, const float* norms, const BatchSlots& ws, int nq, hipStream_t st) {
        hipLaunchKernelGGL((l2_stage_kernel<_Float16, false>), dim3(nq), dim3(64), 0, st, Q, d, norms, ws);
        return "l2_stage_kernel<binary16>";
    }
};

}  // namespace l2sq16
}  // namespace wise

using namespace wise;
using namespace wise::l2sq16;

extern "C" size_t wise_l2sqfp16_topk_workspace_bytes(int64_t N, int d, int nq, int k) { return topk_workspace_bytes(N, d, nq, k); }

extern "C" int wise_l2sq16_topk(const uint16_t* rows, int64_t N, int d, const float* Q, int nq, int k, const int64_t* ids,
                                int64_t id_base, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream) {
    return topk_entry<MetricL2SQ16>("l2sq16_topk", rows, N, d, false, nullptr, 0, Q, nullptr, nq, k, ids, id_base, outD, outI, workspace,
                                    workspace_bytes, stream);
}

extern "C" int wise_l2sq16_topk_pos(const uint16_t* rows, int64_t N, int d, const int64_t* pos, int64_t n_pos, const float* Q, int nq,
                                    int k, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    return topk_entry<MetricL2SQ16>("l2sq16_topk_pos", rows, N, d, true, pos, n_pos, Q, nullptr, nq, k, ids, id_base, outD, outI, workspace,
                                    workspace_bytes, stream);
}

extern "C" size_t wise_l2sqfp16_range_workspace_bytes(int64_t N, int d, int nq) { return range_workspace(N, d, nq); }

extern "C" int wise_l2sq16_range_count(const uint16_t* rows, int64_t N, int d, const float* Q, int nq, float radius, const uint32_t* keep,
                                       int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    return range_count<MetricL2SQ16>("l2sq16_range_count", rows, N, d, Q, nullptr, nq, radius, keep, counts, workspace, workspace_bytes,
                                     stream);
}

extern "C" int wise_l2sq16_range_fill(const uint16_t* rows, int64_t N, int d, const float* Q, int nq, float radius, const int64_t* ids,
                                      int64_t id_base, const int64_t* lims, float* outD, int64_t* outI, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    return range_fill<MetricL2SQ16>("l2sq16_range_fill", rows, N, d, Q, nullptr, nq, radius, ids, id_base, lims, outD, outI, workspace,
                                    workspace_bytes, stream);
}

// search_grouped, stage 1: ord [nq][N] = the ordered image of -dist of every (query, row), 0 for the rows keep clears
extern "C" int wise_l2sq16_group_scores(const uint16_t* rows, int64_t N, int d, const float* Q, int nq, const uint32_t* keep, uint32_t* ord,
                                        void* stream) {
    return group_scores<MetricL2SQ16>("l2sq16_group_scores", rows, N, d, Q, nullptr, nq, keep, ord, stream);
}

extern "C" int wise_l2sq16_prepare(const uint16_t* rows, int64_t N, int d, float* half, float* norms, void* stream) {
    WISE_CHECK_ARG(shape_ok(d), "l2sq16_prepare: d=%d unsupported (d %% 16 == 0 in [16, 1024])", d);
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll && norms && ((rows && half) || N == 0), "l2sq16_prepare: bad argument");
    WISE_CHECK_ARG(((uintptr_t)rows & 15) == 0 && ((uintptr_t)half & 3) == 0, "l2sq16_prepare: rows must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (N > 0) {
        hipLaunchKernelGGL(l2sq16_half_norm_kernel, dim3(wave_row_grid(N)), dim3(256), 0, st, reinterpret_cast<const unsigned char*>(rows),
                           (long long)N, d, half);
        WISE_LAUNCH_CHECK("l2sq16_half_norm_kernel");
    }
    hipLaunchKernelGGL(l2sq16_max_norm_kernel, dim3(1), dim3(1024), 0, st, half, (long long)N, norms);   // N = 0: norms[0] = 0
    WISE_LAUNCH_CHECK("l2sq16_max_norm_kernel");
    return WISE_OK;
}

extern "C" size_t wise_l2sqfp16_topk_batched_workspace_bytes(int64_t N, int d, int nq, int k) {
    return batched_workspace_bytes<MetricL2SQ16>(N, d, nq, k);
}

extern "C" int wise_l2sq16_topk_batched(const uint16_t* rows, const float* half, const float* norms, int64_t N, int d, const float* Q,
                                        int nq, int k, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI,
                                        int32_t* counters, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = batched_args("l2sq16_topk_batched", rows, N, d, Q, nq, k, outD, outI, norms, workspace, workspace_bytes,
                              wise_l2sqfp16_topk_batched_workspace_bytes(N, d, nq, k)))
        return rc;
    WISE_CHECK_ARG(half, "l2sq16_topk_batched: null pointer");
    WISE_CHECK_ARG(((uintptr_t)half & 3) == 0, "l2sq16_topk_batched: half must be 4-byte aligned");
    return topk_batched<MetricL2SQ16>("l2sq16_topk_batched", rows, rows, half, norms, N, d, Q, nullptr, nq, k, ids, id_base, outD, outI, counters,
                                      workspace, (hipStream_t)stream);
}

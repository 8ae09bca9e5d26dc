// HP-2: IndexFlatL2 — exhaustive squared-L2 search over fp32 rows (faiss IndexFlatL2 under an IndexIDMap).  The index is the
// [N, d] fp32 array IndexFlatIP keeps, 4 d bytes a row.
//   wise_l2_topk_f32           THE EXACT SCAN: dist(q, r) = s_0 of CodecL2 under sq_score_loads (sq_codec.h); the k smallest per query
//   wise_l2_topk_pos_f32       the same over an ascending list of positions (an IDSelector resolved by ivf_select.hip)
//   wise_l2_range_*_f32        count / fill of range_search (range_common.h) over the same distance: a hit iff dist < radius
//   wise_l2_prepare            the bf16 copy of the rows (wise_ip_shadow_bf16), its two norms, and half[r] = |x_r|^2 / 2
//   wise_l2_topk_batched       3 or more queries: threshold, collect on v_mfma_f32_32x32x16_bf16, exact re-scoring — the bits of
//                              wise_l2_topk_f32 by construction
// ONE IDEA THROUGHOUT: the score is the negated distance.  Negating an fp32 value is exact, so the sortable (score, position) keys,
// the tie rule (the lower position wins), the per-wave threshold lists and merge_keys_kernel (ip_topk.hip) run unchanged on
// score = -dist; the sign flips back in l2_flip_kernel behind the merge, where merge_keys_kernel's padding -3.4028235e38 becomes
// faiss's L2 padding +3.4028235e38.  dist is a sum of squares from +0, never -0, so score is -0 or negative and flips back to +0.
// The scans, the range pair and the batched search are flat_codec_scan.h's under the policy MetricL2 below (how a wave-load is
// laid out: there; a pass reads N d 4 bytes, what wise_ip_topk_f32 reads).  Here: the policy, the kernels that belong to this type
// alone and the entry points.
#include "flat_codec_scan.h"

namespace wise {
namespace l2 {

using namespace flat_codec;

// behind the merge: the scores of n outputs become distances again (exact; the padding becomes +3.4028235e38)
__global__ __launch_bounds__(256) void l2_flip_kernel(float* __restrict__ D, int n, const int* __restrict__ gate) {
    if (gate && *gate == 0) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) D[i] = -D[i];
}

// wise_l2_prepare: half[r] = 0.5f * |x_r|^2.  One wave per row at a time; lane l runs s = fmaf(x, x, s) over the elements of the
// row's 16-byte pieces l, l + 64, ... in ascending order from +0, the lanes are folded by wave_sum's butterfly (lane masks 32, 16,
// 8, 4, 2, 1) and the sum is halved (exact): a row's half-norm depends on the row alone.
__global__ __launch_bounds__(256) void l2_half_norm_kernel(const float* __restrict__ X, long long N, int d, float* __restrict__ half) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pieces = d >> 2;
    for (long long r = (long long)blockIdx.x * 4 + wave; r < N; r += (long long)gridDim.x * 4) {
        const float4* src = reinterpret_cast<const float4*>(X + (size_t)r * d);
        float s = 0.f;
        for (int p = lane; p < pieces; p += 64) {
            const float4 x = src[p];
            s = fmaf(x.x, x.x, s);
            s = fmaf(x.y, x.y, s);
            s = fmaf(x.z, x.z, s);
            s = fmaf(x.w, x.w, s);
        }
        s = wave_sum(s);
        if (lane == 0) half[r] = 0.5f * s;
    }
}

// ---- the batched search (wise_l2_topk_batched): the pass of flat_codec_scan.h in its threshold form for distances —
// l2_stage_kernel<bf16_t, true> and threshold_above there: the bf16 image of the queries against the bf16 copy of the rows, whose
// rounding (norms[1]) is part of eps.

// THE POLICY (flat_codec_scan.h): the keys order the negated distance, smaller distances are better
struct MetricL2 : PlainPolicy {
    using Codec = CodecL2;
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
    using Piece = bf16x8;
    static __device__ __forceinline__ f32x16 mfma(Piece a, Piece b, f32x16 acc) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
    static constexpr bool HALF_NORMS = true;
    static __device__ __forceinline__ bool candidate(float hv, float acc, float thr) { return !(hv - acc > thr); }
    static const char* stage(const float* Q, int d, const float* norms, const BatchSlots& ws, int nq, hipStream_t st) {
        hipLaunchKernelGGL((l2_stage_kernel<bf16_t, true>), dim3(nq), dim3(64), 0, st, Q, d, norms, ws);
        return "l2_stage_kernel<bf16>";
    }
};

}  // namespace l2

int l2_flip_launch(float* D, int n, const int* gate, hipStream_t st) {
    hipLaunchKernelGGL(l2::l2_flip_kernel, dim3((n + 255) / 256), dim3(256), 0, st, D, n, gate);
    WISE_LAUNCH_CHECK("l2_flip_kernel");
    return WISE_OK;
}

}  // namespace wise

using namespace wise;
using namespace wise::l2;

extern "C" size_t wise_l2_topk_workspace_bytes(int64_t N, int d, int nq, int k) { return topk_workspace_bytes(N, d, nq, k); }

extern "C" int wise_l2_topk_f32(const float* X, int64_t N, int d, const float* Q, int nq, int k, const int64_t* ids, int64_t id_base,
                                float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream) {
    return topk_entry<MetricL2>("l2_topk_f32", X, N, d, false, nullptr, 0, Q, nullptr, nq, k, ids, id_base, outD, outI, workspace, workspace_bytes,
                                stream);
}

extern "C" int wise_l2_topk_pos_f32(const float* X, int64_t N, int d, const int64_t* pos, int64_t n_pos, const float* Q, int nq, int k,
                                    const int64_t* ids, int64_t id_base, float* outD, int64_t* outI, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    return topk_entry<MetricL2>("l2_topk_pos_f32", X, N, d, true, pos, n_pos, Q, nullptr, nq, k, ids, id_base, outD, outI, workspace,
                                workspace_bytes, stream);
}

extern "C" size_t wise_l2_range_workspace_bytes(int64_t N, int d, int nq) { return range_workspace(N, d, nq); }

extern "C" int wise_l2_range_count_f32(const float* X, int64_t N, int d, const float* Q, int nq, float radius, const uint32_t* keep,
                                       int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    return range_count<MetricL2>("l2_range_count_f32", X, N, d, Q, nullptr, nq, radius, keep, counts, workspace, workspace_bytes, stream);
}

extern "C" int wise_l2_range_fill_f32(const float* X, int64_t N, int d, const float* Q, int nq, float radius, const int64_t* ids,
                                      int64_t id_base, const int64_t* lims, float* outD, int64_t* outI, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    return range_fill<MetricL2>("l2_range_fill_f32", X, N, d, Q, nullptr, nq, radius, ids, id_base, lims, outD, outI, workspace, workspace_bytes,
                                stream);
}

// search_grouped, stage 1: ord [nq][N] = the ordered image of -dist of every (query, row), 0 for the rows keep clears
extern "C" int wise_l2_group_scores_f32(const float* X, int64_t N, int d, const float* Q, int nq, const uint32_t* keep, uint32_t* ord,
                                        void* stream) {
    return group_scores<MetricL2>("l2_group_scores_f32", X, N, d, Q, nullptr, nq, keep, ord, stream);
}

extern "C" int wise_l2_prepare(const float* X, int64_t N, int d, uint16_t* Xb, float* half, float* norms, void* stream) {
    WISE_CHECK_ARG(shape_ok(d), "l2_prepare: d=%d unsupported (d %% 16 == 0 in [16, 1024])", d);
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll && norms && ((X && Xb && half) || N == 0), "l2_prepare: bad argument");
    WISE_CHECK_ARG(((uintptr_t)X & 15) == 0 && ((uintptr_t)Xb & 15) == 0, "l2_prepare: X and Xb must be 16-byte aligned");
    if (int rc = wise_ip_shadow_bf16(X, N, d, Xb, norms, stream)) return rc;        // the copy and the two norms
    return wise_l2_half_norms(X, N, d, half, stream);
}

// half[r] of wise_l2_prepare alone: the h_c of the L2 coarse rule (wise_ivf_l2_coarse) over a centroid table
extern "C" int wise_l2_half_norms(const float* X, int64_t N, int d, float* half, void* stream) {
    WISE_CHECK_ARG(shape_ok(d), "l2_half_norms: d=%d unsupported (d %% 16 == 0 in [16, 1024])", d);
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll && ((X && half) || N == 0), "l2_half_norms: bad argument");
    WISE_CHECK_ARG(((uintptr_t)X & 15) == 0, "l2_half_norms: X must be 16-byte aligned");
    if (N == 0) return WISE_OK;
    hipLaunchKernelGGL(l2_half_norm_kernel, dim3(wave_row_grid(N)), dim3(256), 0, (hipStream_t)stream, X, (long long)N, d, half);
    WISE_LAUNCH_CHECK("l2_half_norm_kernel");
    return WISE_OK;
}

extern "C" size_t wise_l2_topk_batched_workspace_bytes(int64_t N, int d, int nq, int k) {
    return batched_workspace_bytes<MetricL2>(N, d, nq, k);
}

extern "C" int wise_l2_topk_batched(const float* X, const uint16_t* Xb, const float* half, const float* norms, int64_t N, int d,
                                    const float* Q, int nq, int k, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI,
                                    int32_t* counters, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = batched_args("l2_topk_batched", X, N, d, Q, nq, k, outD, outI, norms, workspace, workspace_bytes,
                              wise_l2_topk_batched_workspace_bytes(N, d, nq, k)))
        return rc;
    WISE_CHECK_ARG(Xb && half, "l2_topk_batched: null pointer");
    WISE_CHECK_ARG(((uintptr_t)Xb & 15) == 0 && ((uintptr_t)half & 3) == 0, "l2_topk_batched: Xb must be 16-byte aligned");
    return topk_batched<MetricL2>("l2_topk_batched", X, Xb, half, norms, N, d, Q, nullptr, nq, k, ids, id_base, outD, outI, counters, workspace,
                                  (hipStream_t)stream);
}

// The LayerNorm of one fp32 row as the row kernels between the GEMMs compute it (vit.hip, gemm_bf16.hip's fused split-K
// reduction): exact two-pass statistics, the row held in registers as float4s.  The arithmetic is stated ONCE, here: the
// towers' forms (one stream, two half batches, two batches in flight; split-K path and tile path of a text query) must give
// a row the same bits, so every kernel takes its sums, its mean / rstd and its affine from these expression trees.
#pragma once
#include <type_traits>
#include <utility>

#include "common.h"

namespace wise {

__device__ __forceinline__ float ln_sum4(const float4& v) { return (v.x + v.y) + (v.z + v.w); }
// sum of the squared deviations of one float4 from the row's mean
__device__ __forceinline__ float ln_sqdev4(const float4& v, float mean) {
    const float a0 = v.x - mean, a1 = v.y - mean, a2 = v.z - mean, a3 = v.w - mean;
    return (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
}
// (divisions, not multiplications by 1 / W: other last bits)
__device__ __forceinline__ float ln_mean(float s, int W) { return s / (float)W; }
__device__ __forceinline__ float ln_rstd(float q, int W, float eps) { return rsqrtf(q / (float)W + eps); }
__device__ __forceinline__ float4 ln_affine4(const float4& v, float mean, float rstd, const float4& w, const float4& b) {
    return make_float4((v.x - mean) * rstd * w.x + b.x, (v.y - mean) * rstd * w.y + b.y,
                       (v.z - mean) * rstd * w.z + b.z, (v.w - mean) * rstd * w.w + b.w);
}
__device__ __forceinline__ uint2 ln_pack4(const float4& v) { return make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w)); }

// One row per wave: lane l holds the float4 columns l, l + 64, ... (NV of them, zero past the row's w4 = W / 4 columns) and
// adds their sums one after the other before the butterfly.
template <int NV>
struct LnRow {
    float4 v[NV];
    float mean, rstd;

    // mean and rstd of the values held, whose per-lane sum is s
    __device__ __forceinline__ void finish(int lane, int w4, int W, float eps, float s) {
        mean = ln_mean(wave_sum(s), W);
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i)
            if (i * 64 + lane < w4) q += ln_sqdev4(v[i], mean);
        rstd = ln_rstd(wave_sum(q), W, eps);
    }
    // load(c) -> float4 column c of the row
    template <class Load>
    __device__ __forceinline__ void stats(int lane, int w4, int W, float eps, Load load) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = i * 64 + lane;
            v[i] = (c < w4) ? load(c) : make_float4(0.f, 0.f, 0.f, 0.f);
            s += ln_sum4(v[i]);
        }
        finish(lane, w4, W, eps, s);
    }
    // the row becomes (v - mean) * rstd * w + b; store(c, float4) gets each column
    template <class Store>
    __device__ __forceinline__ void affine(int lane, int w4, const float* __restrict__ w, const float* __restrict__ b, Store store) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = i * 64 + lane;
            if (c < w4) {
                v[i] = ln_affine4(v[i], mean, rstd, reinterpret_cast<const float4*>(w)[c], reinterpret_cast<const float4*>(b)[c]);
                store(c, v[i]);
            }
        }
    }
    // the statistics of the row as it now stands (after affine: those of the normalised row, for the LayerNorm fold)
    __device__ __forceinline__ void restat(int lane, int w4, int W, float eps) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i)
            if (i * 64 + lane < w4) s += ln_sum4(v[i]);
        finish(lane, w4, W, eps, s);
    }
};

// Host: f(std::integral_constant<int, nv>()) for 1 <= nv <= MAX, the float4s per lane a width takes; false = not served.
template <class F, int... I>
inline bool with_nv_seq(int nv, F&& f, std::integer_sequence<int, I...>) {
    return ((nv == I + 1 ? (f(std::integral_constant<int, I + 1>()), true) : false) || ...);
}
template <int MAX, class F>
inline bool with_nv(int nv, F&& f) {
    return with_nv_seq(nv, f, std::make_integer_sequence<int, MAX>());
}

}  // namespace wise

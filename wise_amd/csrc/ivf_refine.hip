// HP-2: the re-ranking stage of IndexIVFPQ<m>R8 / IndexIVFPQ<m>R16 (faiss IndexRefine over an IndexIVFPQ).
//   wise_ivf_refine        the kc <= 2048 candidate positions a PQ scan returns are scored again from compact rows kept in list
//                          order (int8 + per-row scale, or bf16: what wise_ip_shadow_i8 / wise_ip_shadow_bf16 build), k best kept
//   wise_ivf_refine_local  the same over ONE RANK's slice of the store of an index sharded across GPUs: the candidates are
//                          positions in the whole array, those outside the slice are holes (one kernel body, pos_base = 0 above)
//   wise_ivf_refine_rows   reconstruct_batch: the dequantised row at a position
// The stage reads kc * d (or 2 d) bytes per query — 51 KB at kc = 100, d = 512 — from rows scattered over the store: it is bound
// by latency, not by HBM.  One workgroup per query: the query goes to LDS, a thread takes a candidate and walks its row in
// 16-byte loads (the query values are LDS broadcasts), the (score, position) keys of the existing scans are sorted in LDS by
// the whole workgroup and the first k are written.
// The score is ONE index-ordered chain of separately rounded products and sums (include/wise_hip.h): contraction is switched
// off in score_row, so no v_fma / v_fmac may appear there — a float32 loop on the host gives the same bits.
#include "topk_common.h"

namespace wise {
namespace ivf_refine {

constexpr int MAX_KC = 2048;
constexpr int MAX_D = 1024;
constexpr int THREADS = 256;

// acc = acc + q[i] * x_i for the 16 values of one 16-byte load of an int8 row, i ascending
__device__ __forceinline__ float chain_i8(float acc, const uint4 w, const float* __restrict__ q) {
#pragma clang fp contract(off)
    const unsigned words[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int v = (int)(signed char)((words[e >> 2] >> (8 * (e & 3))) & 255u);
        const float p = q[e] * (float)v;
        acc = acc + p;
    }
    return acc;
}

// the same for the 8 values of one 16-byte load of a bf16 row (element 0 in the low half of the first word)
__device__ __forceinline__ float chain_bf16(float acc, const uint4 w, const float* __restrict__ q) {
#pragma clang fp contract(off)
    const unsigned words[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const unsigned word = words[e >> 1];
        const float x = __uint_as_float((e & 1) ? (word & 0xFFFF0000u) : (word << 16));
        const float p = q[e] * x;
        acc = acc + p;
    }
    return acc;
}

template <int KIND>
__device__ __forceinline__ float score_row(const unsigned char* __restrict__ rows, const float* __restrict__ scales, long long r, int d,
                                           const float* __restrict__ qs) {
#pragma clang fp contract(off)
    float acc = 0.f;
    if constexpr (KIND == 8) {
        const uint4* row = reinterpret_cast<const uint4*>(rows + (size_t)r * d);
        for (int c = 0; c < (d >> 4); ++c) acc = chain_i8(acc, row[c], qs + 16 * c);
        acc = scales[r] * acc;
    } else {
        const uint4* row = reinterpret_cast<const uint4*>(rows + (size_t)r * d * 2);
        for (int c = 0; c < (d >> 3); ++c) acc = chain_bf16(acc, row[c], qs + 8 * c);
    }
    return acc;
}

// sort buf[0..cap) descending by the whole workgroup (cap = power of two)
__device__ inline void block_bitonic_desc(u64* buf, int cap) {
    for (int size = 2; size <= cap; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (cap >> 1); t += blockDim.x) {
                const int pos = ((t / stride) * (stride << 1)) + (t % stride);
                const int par = pos + stride;
                const bool desc = ((pos & size) == 0);
                const u64 a = buf[pos], b = buf[par];
                const bool sw = desc ? (a < b) : (a > b);
                if (sw) { buf[pos] = b; buf[par] = a; }
            }
            __syncthreads();
        }
    }
}

// block = query.  rows / scales / ids hold positions [pos_base, pos_base + N) of the whole array; cand are positions in the whole
// array; keys carry the local row (within a slice the order of local rows is the order of positions)
template <int KIND>
__global__ __launch_bounds__(THREADS) void refine_kernel(const unsigned char* __restrict__ rows, const float* __restrict__ scales,
                                                         long long N, int d, const long long* __restrict__ ids,
                                                         const float* __restrict__ Q, const long long* __restrict__ cand, int kc,
                                                         int cap, int k, float* __restrict__ outD, long long* __restrict__ outI,
                                                         long long pos_base) {
    __shared__ __attribute__((aligned(16))) float qs[MAX_D];
    __shared__ u64 keys[MAX_KC];
    const int q = blockIdx.x;
    for (int i = threadIdx.x; i < d; i += THREADS) qs[i] = Q[(size_t)q * d + i];
    __syncthreads();
    for (int c = threadIdx.x; c < cap; c += THREADS) {
        u64 key = 0;
        if (c < kc) {
            const long long p = cand[(size_t)q * kc + c];
            if (p >= pos_base && p - pos_base < N) {
                const long long r = p - pos_base;
                key = make_key(score_row<KIND>(rows, scales, r, d, qs), (unsigned)r);
            }
        }
        keys[c] = key;
    }
    __syncthreads();
    block_bitonic_desc(keys, cap);
    for (int i = threadIdx.x; i < k; i += THREADS) {
        const u64 key = i < cap ? keys[i] : 0;
        float s = -3.4028235e38f;
        long long id = -1;
        if (key != 0) {
            const long long r = (long long)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
            s = f32_unorder((unsigned)(key >> 32));
            id = ids ? ids[r] : pos_base + r;
        }
        outD[(size_t)q * k + i] = s;
        outI[(size_t)q * k + i] = id;
    }
}

// block = output row
template <int KIND>
__global__ __launch_bounds__(THREADS) void rows_kernel(const unsigned char* __restrict__ rows, const float* __restrict__ scales,
                                                       long long N, int d, const long long* __restrict__ pos,
                                                       float* __restrict__ out) {
#pragma clang fp contract(off)
    const long long r = pos[blockIdx.x];
    float* o = out + (size_t)blockIdx.x * d;
    if (r < 0 || r >= N) {
        for (int c = threadIdx.x; c < d; c += THREADS) o[c] = __builtin_nanf("");
        return;
    }
    if constexpr (KIND == 8) {
        const signed char* row = reinterpret_cast<const signed char*>(rows) + (size_t)r * d;
        const float s = scales[r];
        for (int c = threadIdx.x; c < d; c += THREADS) o[c] = s * (float)row[c];
    } else {
        const unsigned short* row = reinterpret_cast<const unsigned short*>(rows) + (size_t)r * d;
        for (int c = threadIdx.x; c < d; c += THREADS) o[c] = bf16_to_f32(row[c]);
    }
}

static bool store_shape_ok(int kind, int d) {
    if (kind == 8) return d >= 16 && d <= MAX_D && d % 16 == 0;
    if (kind == 16) return d >= 8 && d <= MAX_D && d % 8 == 0;
    return false;
}

}  // namespace ivf_refine
}  // namespace wise

using namespace wise;
using namespace wise::ivf_refine;

#define REFINE_CHECK_STORE(what)                                                                                                  \
    do {                                                                                                                          \
        if (!store_shape_ok(kind, d)) {                                                                                           \
            set_error(what ": kind=%d d=%d unsupported (kind 8: d %% 16 == 0 in [16, 1024]; kind 16: d %% 8 == 0 in [8, 1024])",    \
                      kind, d);                                                                                                   \
            return WISE_E_UNSUPPORTED;                                                                                            \
        }                                                                                                                         \
    } while (0)

static int refine_impl(const char* what, const void* rows, int kind, const float* scales, int64_t N, int d, const int64_t* ids,
                       const float* Q, int nq, const int64_t* cand_pos, int kc, int k, int64_t pos_base, float* outD, int64_t* outI,
                       void* stream) {
    if (!store_shape_ok(kind, d)) {
        set_error("%s: kind=%d d=%d unsupported (kind 8: d %% 16 == 0 in [16, 1024]; kind 16: d %% 8 == 0 in [8, 1024])", what, kind, d);
        return WISE_E_UNSUPPORTED;
    }
    if (kc < 1 || kc > MAX_KC || k < 1 || k > MAX_KC) {
        set_error("%s: kc=%d k=%d unsupported (both in [1, %d])", what, kc, k, MAX_KC);
        return WISE_E_UNSUPPORTED;
    }
    WISE_CHECK_ARG(nq >= 0 && N >= 0 && N < 0xFFFFFFFFll && pos_base >= 0, "%s: nq=%d N=%lld pos_base=%lld out of range", what, nq,
                   (long long)N, (long long)pos_base);
    if (nq == 0) return WISE_OK;
    WISE_CHECK_ARG(Q && cand_pos && outD && outI && (N == 0 || (rows && (kind == 16 || scales))), "%s: null pointer", what);
    WISE_CHECK_ARG(((uintptr_t)rows & 15) == 0, "%s: rows must be 16-byte aligned", what);
    int cap = 64;
    while (cap < kc) cap <<= 1;
    const unsigned char* r8 = reinterpret_cast<const unsigned char*>(rows);
    const long long* id = reinterpret_cast<const long long*>(ids);
    const long long* cp = reinterpret_cast<const long long*>(cand_pos);
    long long* oi = reinterpret_cast<long long*>(outI);
    if (kind == 8)
        hipLaunchKernelGGL(refine_kernel<8>, dim3(nq), dim3(THREADS), 0, (hipStream_t)stream, r8, scales, (long long)N, d, id, Q, cp, kc,
                           cap, k, outD, oi, (long long)pos_base);
    else
        hipLaunchKernelGGL(refine_kernel<16>, dim3(nq), dim3(THREADS), 0, (hipStream_t)stream, r8, scales, (long long)N, d, id, Q, cp, kc,
                           cap, k, outD, oi, (long long)pos_base);
    WISE_LAUNCH_CHECK("ivf refine_kernel");
    return WISE_OK;
}

extern "C" int wise_ivf_refine(const void* rows, int kind, const float* scales, int64_t N, int d, const int64_t* ids, const float* Q,
                               int nq, const int64_t* cand_pos, int kc, int k, float* outD, int64_t* outI, void* stream) {
    return refine_impl("ivf_refine", rows, kind, scales, N, d, ids, Q, nq, cand_pos, kc, k, 0, outD, outI, stream);
}

extern "C" int wise_ivf_refine_local(const void* rows, int kind, const float* scales, int64_t N, int d, const int64_t* ids,
                                     const float* Q, int nq, const int64_t* cand_pos, int kc, int k, int64_t pos_base, float* outD,
                                     int64_t* outI, void* stream) {
    return refine_impl("ivf_refine_local", rows, kind, scales, N, d, ids, Q, nq, cand_pos, kc, k, pos_base, outD, outI, stream);
}

extern "C" int wise_ivf_refine_rows(const void* rows, int kind, const float* scales, int64_t N, int d, const int64_t* pos, int n,
                                    float* out, void* stream) {
    REFINE_CHECK_STORE("ivf_refine_rows");
    WISE_CHECK_ARG(n >= 0 && N >= 0 && (n == 0 || (pos && out)) && (N == 0 || (rows && (kind == 16 || scales))),
                   "ivf_refine_rows: bad argument");
    if (n == 0) return WISE_OK;
    const unsigned char* r8 = reinterpret_cast<const unsigned char*>(rows);
    const long long* p = reinterpret_cast<const long long*>(pos);
    if (kind == 8)
        hipLaunchKernelGGL(rows_kernel<8>, dim3(n), dim3(THREADS), 0, (hipStream_t)stream, r8, scales, (long long)N, d, p, out);
    else
        hipLaunchKernelGGL(rows_kernel<16>, dim3(n), dim3(THREADS), 0, (hipStream_t)stream, r8, scales, (long long)N, d, p, out);
    WISE_LAUNCH_CHECK("ivf refine rows_kernel");
    return WISE_OK;
}

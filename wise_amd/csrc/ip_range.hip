// ------------------------------------------------------------------------------------------------
// range_search on the fp32 rows (wise_ip_range_*, wise_ivf_range_*): every row with score > radius, the score being
// row_partials / rows_reduce (topk_common.h) — the bits ip_scan_kernel (ip_topk.hip) gives that row.  Structure, workspace and the determinism
// argument: range_common.h.  Groups of 4 rows as the scan; a group is one 16 d-byte burst, 16 B per lane per load.
// ------------------------------------------------------------------------------------------------
#include "range_common.h"

namespace wise {

constexpr int RANGE_R = 4;

template <int NV, int NQ>
__device__ __forceinline__ void range_load_queries(const float* __restrict__ Q, int d4, int q0, int nq, int lane, float4 (&qv)[NQ][NV]) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int qi = q0 + q < nq ? q0 + q : nq - 1;   // a ragged tile repeats the last query; its results are not written
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int c = v * 64 + lane;
            qv[q][v] = (c < d4) ? reinterpret_cast<const float4*>(Q)[(long long)qi * d4 + c] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

template <int NV>
__device__ __forceinline__ void range_load_rows(const f32x4* __restrict__ X, int d4, const long long (&row)[RANGE_R], int lane,
                                                f32x4 (&x)[RANGE_R][NV]) {
#pragma unroll
    for (int r = 0; r < RANGE_R; ++r)
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int c = v * 64 + lane;
            if (NV * 64 == d4 || c < d4)
                x[r][v] = __builtin_nontemporal_load(&X[row[r] * d4 + c]);
            else
                x[r][v] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
}

// the rows [clo, chi) (at most RANGE_ROWS) against NQ queries: bit (row - clo) of hb[q] is set where score > radius.  A group
// whose rows are all cleared in keep is not loaded (wave-uniform).  The four waves take the groups round-robin.
template <int NV, int NQ>
__device__ __forceinline__ void range_mark_chunk(const f32x4* __restrict__ X, int d4, const float4 (&qv)[NQ][NV], long long clo,
                                                 long long chi, float radius, const unsigned* __restrict__ keep,
                                                 unsigned (*hb)[RANGE_WORDS]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int myr = reduced_row<RANGE_R>(lane);
    const bool owner = (lane & 15) == 0;
    const int ngroups = (int)((chi - clo + RANGE_R - 1) / RANGE_R);
    for (int g = wave; g < ngroups; g += 4) {
        const long long row0 = clo + (long long)g * RANGE_R;
        const long long mine = row0 + myr;
        bool chosen = mine < chi;
        if (keep) {
            chosen = chosen && ((keep[mine >> 5] >> (mine & 31)) & 1u) != 0;
            if (__ballot(chosen) == 0) continue;
        }
        long long row[RANGE_R];
#pragma unroll
        for (int r = 0; r < RANGE_R; ++r) row[r] = row0 + r < chi ? row0 + r : chi - 1;   // stay in bounds; masked by chosen
        f32x4 x[RANGE_R][NV];
        range_load_rows<NV>(X, d4, row, lane, x);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            float a[RANGE_R];
            row_partials<NV, RANGE_R>(x, qv[q], a);
            const float s = rows_reduce<RANGE_R>(a, lane);
            if (owner && chosen && s > radius) range_mark(hb[q], (int)(mine - clo));
        }
    }
}

// flat count: block (x, y) owns segment x = rows [x RANGE_ROWS, ...) for the queries y NQ .. y NQ + NQ - 1
template <int NV, int NQ>
__global__ __launch_bounds__(256) void ip_range_count_kernel(const f32x4* __restrict__ X, long long N, int d4,
                                                             const float* __restrict__ Q, int nq, float radius,
                                                             const unsigned* __restrict__ keep, unsigned* __restrict__ hit,
                                                             long long wstride, long long* __restrict__ seg, long long ns) {
    __shared__ unsigned hb[NQ][RANGE_WORDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q0 = blockIdx.y * NQ;
    float4 qv[NQ][NV];
    range_load_queries<NV, NQ>(Q, d4, q0, nq, lane, qv);
    for (int i = threadIdx.x; i < NQ * RANGE_WORDS; i += 256) hb[i / RANGE_WORDS][i % RANGE_WORDS] = 0u;
    __syncthreads();
    const long long clo = (long long)blockIdx.x * RANGE_ROWS;
    const long long chi = clo + RANGE_ROWS < N ? clo + RANGE_ROWS : N;
    range_mark_chunk<NV, NQ>(X, d4, qv, clo, chi, radius, keep, hb);
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            if (q0 + q >= nq) break;
            const int n = range_publish(hb[q], hit + (size_t)(q0 + q) * wstride + (size_t)blockIdx.x * RANGE_WORDS, RANGE_WORDS, lane);
            if (lane == 0) seg[(size_t)(q0 + q) * (ns + 1) + blockIdx.x] = n;
        }
    }
}

// ---- search_grouped, stage 1 (group_topk.hip holds stages 2 and 3): the count kernels with the hit mark replaced by one store.
// range_mark_chunk with sc[q][row - clo] = f32_order(score) in place of the mark — the upper half of the key ip_scan_kernel makes
// of that (query, row).  sc is cleared by the caller: a row cleared in keep reads 0, the keys' empty value.
template <int NV, int NQ>
__device__ __forceinline__ void group_score_chunk(const f32x4* __restrict__ X, int d4, const float4 (&qv)[NQ][NV], long long clo,
                                                  long long chi, const unsigned* __restrict__ keep, unsigned (*sc)[RANGE_ROWS]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int myr = reduced_row<RANGE_R>(lane);
    const bool owner = (lane & 15) == 0;
    const int ngroups = (int)((chi - clo + RANGE_R - 1) / RANGE_R);
    for (int g = wave; g < ngroups; g += 4) {
        const long long row0 = clo + (long long)g * RANGE_R;
        const long long mine = row0 + myr;
        bool chosen = mine < chi;
        if (keep) {
            chosen = chosen && ((keep[mine >> 5] >> (mine & 31)) & 1u) != 0;
            if (__ballot(chosen) == 0) continue;
        }
        long long row[RANGE_R];
#pragma unroll
        for (int r = 0; r < RANGE_R; ++r) row[r] = row0 + r < chi ? row0 + r : chi - 1;   // stay in bounds; masked by chosen
        f32x4 x[RANGE_R][NV];
        range_load_rows<NV>(X, d4, row, lane, x);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            float a[RANGE_R];
            row_partials<NV, RANGE_R>(x, qv[q], a);
            const float s = rows_reduce<RANGE_R>(a, lane);
            if (owner && chosen) sc[q][(int)(mine - clo)] = f32_order(s);
        }
    }
}

// the images of the rows [clo, chi) leave LDS as one run of 4-byte words per query: every row of the chunk is written
template <int NQ>
__device__ __forceinline__ void group_publish(const unsigned (*sc)[RANGE_ROWS], unsigned* __restrict__ ord, long long N, int q0, int nq,
                                              long long clo, long long chi) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        if (q0 + q >= nq) break;
        unsigned* dst = ord + (size_t)(q0 + q) * (size_t)N + (size_t)clo;
        for (int i = threadIdx.x; i < (int)(chi - clo); i += 256) dst[i] = sc[q][i];
    }
}

// flat: block (x, y) owns segment x = rows [x RANGE_ROWS, ...) for the queries y NQ .. y NQ + NQ - 1, as ip_range_count_kernel
template <int NV, int NQ>
__global__ __launch_bounds__(256) void ip_group_scores_kernel(const f32x4* __restrict__ X, long long N, int d4, const float* __restrict__ Q,
                                                              int nq, const unsigned* __restrict__ keep, unsigned* __restrict__ ord) {
    __shared__ unsigned sc[NQ][RANGE_ROWS];
    const int lane = threadIdx.x & 63;
    const int q0 = blockIdx.y * NQ;
    float4 qv[NQ][NV];
    range_load_queries<NV, NQ>(Q, d4, q0, nq, lane, qv);
    for (int i = threadIdx.x; i < NQ * RANGE_ROWS; i += 256) sc[i / RANGE_ROWS][i % RANGE_ROWS] = 0u;
    __syncthreads();
    const long long clo = (long long)blockIdx.x * RANGE_ROWS;
    const long long chi = clo + RANGE_ROWS < N ? clo + RANGE_ROWS : N;
    group_score_chunk<NV, NQ>(X, d4, qv, clo, chi, keep, sc);
    __syncthreads();
    group_publish<NQ>(sc, ord, N, q0, nq, clo, chi);
}

struct RangeLists {
    const long long* probes;    // [nq][nprobe], < 0 or >= nlist: nothing to scan
    const long long* list_off;  // [nlist + 1]
    int nprobe, nlist;
};

// inverted-list count: block b owns probe b % nprobe of query b / nprobe, as ip_scan_kernel<SEG>
template <int NV>
__global__ __launch_bounds__(256) void ivf_range_count_kernel(const f32x4* __restrict__ X, int d4, const float* __restrict__ Q,
                                                              float radius, const unsigned* __restrict__ keep, RangeLists ls,
                                                              unsigned* __restrict__ hit, long long wstride,
                                                              long long* __restrict__ seg) {
    __shared__ unsigned hb[1][RANGE_WORDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qi = blockIdx.x / ls.nprobe, pi = blockIdx.x - qi * ls.nprobe;
    const long long l = ls.probes[(size_t)qi * ls.nprobe + pi];
    long long lo = 0, hi = 0;
    if (l >= 0 && l < ls.nlist) { lo = ls.list_off[l]; hi = ls.list_off[l + 1]; }   // block-uniform
    float4 qv[1][NV];
    range_load_queries<NV, 1>(Q, d4, qi, qi + 1, lane, qv);
    unsigned* dst = hit + (size_t)qi * wstride + (lo >> 5) + (l > 0 ? l : 0);
    long long total = 0;
    for (long long clo = lo; clo < hi; clo += RANGE_ROWS, dst += RANGE_WORDS) {
        const long long chi = clo + RANGE_ROWS < hi ? clo + RANGE_ROWS : hi;
        if (wave == 0) hb[0][lane] = 0u;
        __syncthreads();
        range_mark_chunk<NV, 1>(X, d4, qv, clo, chi, radius, keep, hb);
        __syncthreads();
        if (wave == 0) total += range_publish(hb[0], dst, (int)((chi - clo + 31) >> 5), lane);
    }
    if (threadIdx.x == 0) seg[(size_t)qi * (ls.nprobe + 1) + pi] = total;
}

// inverted lists: block b owns probe b % nprobe of query b / nprobe, as ivf_range_count_kernel.  Probed lists are distinct, so
// every (query, row) is stored at most once; the rows of the lists a query does not probe are not written (the entry point
// clears ord first)
template <int NV>
__global__ __launch_bounds__(256) void ivf_group_scores_kernel(const f32x4* __restrict__ X, long long N, int d4, const float* __restrict__ Q,
                                                               const unsigned* __restrict__ keep, RangeLists ls, unsigned* __restrict__ ord) {
    __shared__ unsigned sc[1][RANGE_ROWS];
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x / ls.nprobe, pi = blockIdx.x - qi * ls.nprobe;
    const long long l = ls.probes[(size_t)qi * ls.nprobe + pi];
    long long lo = 0, hi = 0;
    if (l >= 0 && l < ls.nlist) { lo = ls.list_off[l]; hi = ls.list_off[l + 1]; }   // block-uniform
    if (lo < 0) lo = 0;
    if (hi > N) hi = N;                                                             // never past ord's row, whatever list_off holds
    float4 qv[1][NV];
    range_load_queries<NV, 1>(Q, d4, qi, qi + 1, lane, qv);
    for (long long clo = lo; clo < hi; clo += RANGE_ROWS) {
        const long long chi = clo + RANGE_ROWS < hi ? clo + RANGE_ROWS : hi;
        for (int i = threadIdx.x; i < RANGE_ROWS; i += 256) sc[0][i] = 0u;
        __syncthreads();
        group_score_chunk<NV, 1>(X, d4, qv, clo, chi, keep, sc);
        __syncthreads();
        group_publish<1>(sc, ord, N, qi, qi + 1, clo, chi);
        __syncthreads();
    }
}

// fill, both forms: the hits of one segment, in ascending position, behind lims[q] + the segment's offset.
// SEG = false: grid (ns, nq), segment = RANGE_ROWS rows; SEG = true: grid nq * nprobe, segment = a probed list.
template <int NV, bool SEG>
__global__ __launch_bounds__(256) void range_fill_kernel(const f32x4* __restrict__ X, long long N, int d4, const float* __restrict__ Q,
                                                         const long long* __restrict__ ids, long long id_base, RangeLists ls,
                                                         const unsigned* __restrict__ hit, long long wstride,
                                                         const long long* __restrict__ seg, long long ns,
                                                         const long long* __restrict__ lims, float* __restrict__ outD,
                                                         long long* __restrict__ outI) {
    __shared__ unsigned short lst[RANGE_ROWS];
    __shared__ int s_cnt;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int qi, si;
    if constexpr (SEG) { qi = blockIdx.x / ls.nprobe; si = blockIdx.x - qi * ls.nprobe; } else { qi = blockIdx.y; si = blockIdx.x; }
    const long long* so = seg + (size_t)qi * (ns + 1) + si;
    long long left = so[1] - so[0];                              // hits count found in this segment: never more are written
    if (left <= 0) return;                                  // no hit in this segment (block-uniform)
    long long dest = lims[qi] + so[0];
    long long lo, hi;
    const unsigned* words = hit + (size_t)qi * wstride;
    if constexpr (SEG) {
        const long long l = ls.probes[(size_t)qi * ls.nprobe + si];
        if (l < 0 || l >= ls.nlist) return;                            // not the probes count saw: nothing to read
        lo = ls.list_off[l]; hi = ls.list_off[l + 1];
        words += (lo >> 5) + l;
    } else {
        lo = (long long)si * RANGE_ROWS;
        hi = lo + RANGE_ROWS < N ? lo + RANGE_ROWS : N;
        words += (size_t)si * RANGE_WORDS;
    }
    float4 qv[1][NV];
    range_load_queries<NV, 1>(Q, d4, qi, qi + 1, lane, qv);
    const int myr = reduced_row<RANGE_R>(lane);
    const bool owner = (lane & 15) == 0;
    for (long long clo = lo; clo < hi; clo += RANGE_ROWS, words += RANGE_WORDS) {
        const long long chi = clo + RANGE_ROWS < hi ? clo + RANGE_ROWS : hi;
        if (wave == 0) {
            const int n = range_list(words, (int)((chi - clo + 31) >> 5), lst, lane);
            if (lane == 0) s_cnt = n;
        }
        __syncthreads();
        const int cnt = s_cnt < left ? s_cnt : (int)left;
        for (int g = wave; g * RANGE_R < cnt; g += 4) {
            long long row[RANGE_R];
#pragma unroll
            for (int r = 0; r < RANGE_R; ++r) {
                const int e = g * RANGE_R + r;
                row[r] = clo + lst[e < cnt ? e : cnt - 1];
            }
            f32x4 x[RANGE_R][NV];
            range_load_rows<NV>(X, d4, row, lane, x);
            float a[RANGE_R];
            row_partials<NV, RANGE_R>(x, qv[0], a);
            const float s = rows_reduce<RANGE_R>(a, lane);
            const int e = g * RANGE_R + myr;
            if (owner && e < cnt) {
                const long long r = clo + lst[e];
                outD[dest + e] = s;
                outI[dest + e] = ids ? ids[r] : id_base + r;
            }
        }
        __syncthreads();
        dest += cnt;
        left -= cnt;
    }
}

template <int NV>
static void launch_ip_range_count(int nqp, const float* X, long long N, int d, const float* Q, int nq, float radius,
                                  const unsigned* keep, unsigned* hit, long long wstride, long long* seg, long long ns, hipStream_t st) {
    const f32x4* X4 = reinterpret_cast<const f32x4*>(X);
    const dim3 grid((unsigned)ns, (unsigned)((nq + nqp - 1) / nqp));
    if constexpr (NV * 4 <= 8) {
        if (nqp == 4) { hipLaunchKernelGGL((ip_range_count_kernel<NV, 4>), grid, dim3(256), 0, st, X4, N, d / 4, Q, nq, radius, keep, hit, wstride, seg, ns); return; }
    }
    if constexpr (NV * 2 <= 8) {
        if (nqp == 2) { hipLaunchKernelGGL((ip_range_count_kernel<NV, 2>), grid, dim3(256), 0, st, X4, N, d / 4, Q, nq, radius, keep, hit, wstride, seg, ns); return; }
    }
    hipLaunchKernelGGL((ip_range_count_kernel<NV, 1>), grid, dim3(256), 0, st, X4, N, d / 4, Q, nq, radius, keep, hit, wstride, seg, ns);
}

// queries that share a pass over the rows: the register rule of plan_scan (NV * NQ <= 8)
static int range_queries_per_pass(int d, int nq) {
    const int nv = (d / 4 + 63) / 64;
    int nqp = 1;
    while (nqp * 2 <= nq && nqp * 2 <= 4 && nv * nqp * 2 <= 8) nqp <<= 1;
    return nqp;
}

#define RANGE_NV_SWITCH(d, CALL)                     \
    switch (((d) / 4 + 63) / 64) {                   \
        case 1: CALL(1); break;                      \
        case 2: CALL(2); break;                      \
        case 3: CALL(3); break;                      \
        case 4: CALL(4); break;                      \
        case 5: CALL(5); break;                      \
        case 6: CALL(6); break;                      \
        case 7: CALL(7); break;                      \
        default: CALL(8); break;                     \
    }

}  // namespace wise

using namespace wise;

static int range_common_args(const char* what, int64_t N, int d, int nq, const void* X, const void* Q, float radius) {
    WISE_CHECK_ARG(d >= 4 && d <= 2048 && d % 4 == 0, "%s: d=%d must be a multiple of 4 in [4,2048]", what, d);
    WISE_CHECK_ARG(nq >= 1 && nq <= 65535, "%s: nq=%d out of [1,65535]", what, nq);
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll, "%s: N=%lld out of range", what, (long long)N);
    WISE_CHECK_ARG(Q && (X || N == 0), "%s: null pointer", what);
    WISE_CHECK_ARG(((uintptr_t)X & 15) == 0 && ((uintptr_t)Q & 15) == 0, "%s: X and Q must be 16-byte aligned", what);
    WISE_CHECK_ARG(radius == radius && radius - radius == 0.f, "%s: radius must be finite", what);
    return WISE_OK;
}

extern "C" size_t wise_ip_range_workspace_bytes(int64_t N, int d, int nq) {
    if (N < 0 || N >= 0xFFFFFFFFll || d < 4 || d > 2048 || d % 4 || nq < 1 || nq > 65535) return 0;
    const long long ns = range_flat_segments(N);
    return range_workspace_bytes(nq, ns * RANGE_WORDS, ns);
}

extern "C" int wise_ip_range_count_f32(const float* X, int64_t N, int d, const float* Q, int nq, float radius, const uint32_t* keep,
                                       int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = range_common_args("ip_range_count", N, d, nq, X, Q, radius)) return rc;
    WISE_CHECK_ARG(counts, "ip_range_count: null pointer");
    const size_t need = wise_ip_range_workspace_bytes(N, d, nq);
    WISE_CHECK_ARG(workspace && workspace_bytes >= need, "ip_range_count: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const long long ns = range_flat_segments(N), wstride = ns * RANGE_WORDS;
    unsigned* hit = reinterpret_cast<unsigned*>(workspace);
    long long* seg = reinterpret_cast<long long*>(reinterpret_cast<unsigned char*>(workspace) + range_hit_bytes(nq, wstride));
    if (ns > 0) {
        const int nqp = range_queries_per_pass(d, nq);
        ProfScope prof(PROF_SCAN, (double)N * d * 4.0 * ((nq + nqp - 1) / nqp), st);
#define CALL(NV) launch_ip_range_count<NV>(nqp, X, N, d, Q, nq, radius, keep, hit, wstride, seg, ns, st)
        RANGE_NV_SWITCH(d, CALL)
#undef CALL
        WISE_LAUNCH_CHECK("ip_range_count_kernel");
    }
    hipLaunchKernelGGL(range_scan_kernel, dim3(nq), dim3(1024), 0, st, seg, ns, reinterpret_cast<long long*>(counts));
    WISE_LAUNCH_CHECK("range_scan_kernel");
    return WISE_OK;
}

extern "C" int wise_ip_range_fill_f32(const float* X, int64_t N, int d, const float* Q, int nq, float radius, const int64_t* ids,
                                      int64_t id_base, const int64_t* lims, float* outD, int64_t* outI, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    if (int rc = range_common_args("ip_range_fill", N, d, nq, X, Q, radius)) return rc;
    WISE_CHECK_ARG(lims && outD && outI, "ip_range_fill: null pointer");
    const size_t need = wise_ip_range_workspace_bytes(N, d, nq);
    WISE_CHECK_ARG(workspace && workspace_bytes >= need, "ip_range_fill: workspace %zu < %zu bytes", workspace_bytes, need);
    const long long ns = range_flat_segments(N), wstride = ns * RANGE_WORDS;
    if (ns == 0) return WISE_OK;
    hipStream_t st = (hipStream_t)stream;
    const unsigned* hit = reinterpret_cast<const unsigned*>(workspace);
    const long long* seg = reinterpret_cast<const long long*>(reinterpret_cast<unsigned char*>(workspace) + range_hit_bytes(nq, wstride));
    const RangeLists none{};
#define CALL(NV)                                                                                                                  \
    hipLaunchKernelGGL((range_fill_kernel<NV, false>), dim3((unsigned)ns, (unsigned)nq), dim3(256), 0, st,                         \
                       reinterpret_cast<const f32x4*>(X), (long long)N, d / 4, Q, reinterpret_cast<const long long*>(ids),        \
                       (long long)id_base, none, hit, wstride, seg, ns, reinterpret_cast<const long long*>(lims), outD,           \
                       reinterpret_cast<long long*>(outI))
    RANGE_NV_SWITCH(d, CALL)
#undef CALL
    WISE_LAUNCH_CHECK("range_fill_kernel");
    return WISE_OK;
}

static bool ivf_range_shape_ok(int64_t N, int nlist, int nq, int nprobe) {
    return N >= 0 && N < 0xFFFFFFFFll && nlist >= 1 && nq >= 1 && nq <= 65535 && nprobe >= 1 && nprobe <= 2048;
}

extern "C" size_t wise_ivf_range_workspace_bytes(int64_t N, int nlist, int nq, int nprobe) {
    if (!ivf_range_shape_ok(N, nlist, nq, nprobe)) return 0;
    return range_workspace_bytes(nq, range_ivf_wstride(N, nlist), nprobe);
}

extern "C" int wise_ivf_range_count_f32(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const float* Q, int nq,
                                        const int64_t* probes, int nprobe, float radius, const uint32_t* keep, int64_t* counts,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = range_common_args("ivf_range_count", N, d, nq, X, Q, radius)) return rc;
    WISE_CHECK_ARG(ivf_range_shape_ok(N, nlist, nq, nprobe), "ivf_range_count: nq=%d nprobe=%d nlist=%d out of range (nq <= 65535, nprobe <= 2048)",
                   nq, nprobe, nlist);
    WISE_CHECK_ARG(counts && list_off && probes, "ivf_range_count: null pointer");
    const size_t need = wise_ivf_range_workspace_bytes(N, nlist, nq, nprobe);
    WISE_CHECK_ARG(workspace && workspace_bytes >= need, "ivf_range_count: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const long long wstride = range_ivf_wstride(N, nlist);
    unsigned* hit = reinterpret_cast<unsigned*>(workspace);
    long long* seg = reinterpret_cast<long long*>(reinterpret_cast<unsigned char*>(workspace) + range_hit_bytes(nq, wstride));
    const RangeLists ls{reinterpret_cast<const long long*>(probes), reinterpret_cast<const long long*>(list_off), nprobe, nlist};
#define CALL(NV)                                                                                                                   \
    hipLaunchKernelGGL((ivf_range_count_kernel<NV>), dim3((unsigned)((long long)nq * nprobe)), dim3(256), 0, st,                   \
                       reinterpret_cast<const f32x4*>(X), d / 4, Q, radius, keep, ls, hit, wstride, seg)
    RANGE_NV_SWITCH(d, CALL)
#undef CALL
    WISE_LAUNCH_CHECK("ivf_range_count_kernel");
    hipLaunchKernelGGL(range_scan_kernel, dim3(nq), dim3(1024), 0, st, seg, (long long)nprobe, reinterpret_cast<long long*>(counts));
    WISE_LAUNCH_CHECK("range_scan_kernel");
    return WISE_OK;
}

extern "C" int wise_ivf_range_fill_f32(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                                       const float* Q, int nq, const int64_t* probes, int nprobe, float radius, const int64_t* lims,
                                       float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = range_common_args("ivf_range_fill", N, d, nq, X, Q, radius)) return rc;
    WISE_CHECK_ARG(ivf_range_shape_ok(N, nlist, nq, nprobe), "ivf_range_fill: nq=%d nprobe=%d nlist=%d out of range (nq <= 65535, nprobe <= 2048)",
                   nq, nprobe, nlist);
    WISE_CHECK_ARG(lims && outD && outI && list_off && probes, "ivf_range_fill: null pointer");
    const size_t need = wise_ivf_range_workspace_bytes(N, nlist, nq, nprobe);
    WISE_CHECK_ARG(workspace && workspace_bytes >= need, "ivf_range_fill: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const long long wstride = range_ivf_wstride(N, nlist);
    const unsigned* hit = reinterpret_cast<const unsigned*>(workspace);
    const long long* seg = reinterpret_cast<const long long*>(reinterpret_cast<unsigned char*>(workspace) + range_hit_bytes(nq, wstride));
    const RangeLists ls{reinterpret_cast<const long long*>(probes), reinterpret_cast<const long long*>(list_off), nprobe, nlist};
#define CALL(NV)                                                                                                                  \
    hipLaunchKernelGGL((range_fill_kernel<NV, true>), dim3((unsigned)((long long)nq * nprobe)), dim3(256), 0, st,                  \
                       reinterpret_cast<const f32x4*>(X), (long long)N, d / 4, Q, reinterpret_cast<const long long*>(ids), 0ll, ls, \
                       hit, wstride, seg, (long long)nprobe, reinterpret_cast<const long long*>(lims), outD,                      \
                       reinterpret_cast<long long*>(outI))
    RANGE_NV_SWITCH(d, CALL)
#undef CALL
    WISE_LAUNCH_CHECK("range_fill_kernel");
    return WISE_OK;
}

// ---- search_grouped, stage 1 over the fp32 rows: ord [nq][N] receives f32_order(score) of every candidate (query, row)
template <int NV>
static void launch_ip_group_scores(int nqp, const float* X, long long N, int d, const float* Q, int nq, const unsigned* keep, unsigned* ord,
                                   long long ns, hipStream_t st) {
    const f32x4* X4 = reinterpret_cast<const f32x4*>(X);
    const dim3 grid((unsigned)ns, (unsigned)((nq + nqp - 1) / nqp));
    if constexpr (NV * 4 <= 8) {
        if (nqp == 4) { hipLaunchKernelGGL((ip_group_scores_kernel<NV, 4>), grid, dim3(256), 0, st, X4, N, d / 4, Q, nq, keep, ord); return; }
    }
    if constexpr (NV * 2 <= 8) {
        if (nqp == 2) { hipLaunchKernelGGL((ip_group_scores_kernel<NV, 2>), grid, dim3(256), 0, st, X4, N, d / 4, Q, nq, keep, ord); return; }
    }
    hipLaunchKernelGGL((ip_group_scores_kernel<NV, 1>), grid, dim3(256), 0, st, X4, N, d / 4, Q, nq, keep, ord);
}

static int group_common_args(const char* what, int64_t N, int d, int nq, const void* X, const void* Q, const void* ord) {
    WISE_CHECK_ARG(d >= 4 && d <= 2048 && d % 4 == 0, "%s: d=%d must be a multiple of 4 in [4,2048]", what, d);
    WISE_CHECK_ARG(nq >= 1 && nq <= 65535, "%s: nq=%d out of [1,65535]", what, nq);
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll, "%s: N=%lld out of range", what, (long long)N);
    WISE_CHECK_ARG(Q && (X || N == 0) && (ord || N == 0), "%s: null pointer", what);
    WISE_CHECK_ARG(((uintptr_t)X & 15) == 0 && ((uintptr_t)Q & 15) == 0, "%s: X and Q must be 16-byte aligned", what);
    return WISE_OK;
}

// the exact fp32 routine of wise_ip_topk_f32 over every row; a row cleared in keep reads 0.  Every row is written: nothing is cleared
extern "C" int wise_ip_group_scores_f32(const float* X, int64_t N, int d, const float* Q, int nq, const uint32_t* keep, uint32_t* ord,
                                        void* stream) {
    if (int rc = group_common_args("ip_group_scores", N, d, nq, X, Q, ord)) return rc;
    const long long ns = range_flat_segments(N);
    if (ns == 0) return WISE_OK;
    hipStream_t st = (hipStream_t)stream;
    const int nqp = range_queries_per_pass(d, nq);
    ProfScope prof(PROF_SCAN, (double)N * d * 4.0 * ((nq + nqp - 1) / nqp), st);
#define CALL(NV) launch_ip_group_scores<NV>(nqp, X, N, d, Q, nq, keep, ord, ns, st)
    RANGE_NV_SWITCH(d, CALL)
#undef CALL
    WISE_LAUNCH_CHECK("ip_group_scores_kernel");
    return WISE_OK;
}

// the rows of the probed lists (wise_ivf_scan_f32's candidates and scores); every other row of ord reads 0: ord is cleared first
extern "C" int wise_ivf_group_scores_f32(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const float* Q, int nq,
                                         const int64_t* probes, int nprobe, const uint32_t* keep, uint32_t* ord, void* stream) {
    if (int rc = group_common_args("ivf_group_scores", N, d, nq, X, Q, ord)) return rc;
    WISE_CHECK_ARG(ivf_range_shape_ok(N, nlist, nq, nprobe), "ivf_group_scores: nq=%d nprobe=%d nlist=%d out of range (nq <= 65535, nprobe <= 2048)",
                   nq, nprobe, nlist);
    WISE_CHECK_ARG(list_off && probes, "ivf_group_scores: null pointer");
    if (N == 0) return WISE_OK;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(ord, 0, (size_t)nq * (size_t)N * sizeof(uint32_t), st);
    if (e != hipSuccess) { set_error("ivf_group_scores: memset: %s", hipGetErrorString(e)); return (int)e; }
    const RangeLists ls{reinterpret_cast<const long long*>(probes), reinterpret_cast<const long long*>(list_off), nprobe, nlist};
#define CALL(NV)                                                                                                                   \
    hipLaunchKernelGGL((ivf_group_scores_kernel<NV>), dim3((unsigned)((long long)nq * nprobe)), dim3(256), 0, st,                  \
                       reinterpret_cast<const f32x4*>(X), (long long)N, d / 4, Q, keep, ls, ord)
    RANGE_NV_SWITCH(d, CALL)
#undef CALL
    WISE_LAUNCH_CHECK("ivf_group_scores_kernel");
    return WISE_OK;
}

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
// The scan is ip_sq16.hip's with CodecL2 in Codec16's place: a row is C = d / 16 chunks, lane (sub, c) of a wave-load holds chunk c
// of row sub, RPL = 64 / C whole rows per load and SQ_T loads in flight; chunk c is the row's 16-byte pieces c, C + c, 2 C + c and
// 3 C + c, so each of a wave-load's four load instructions reads RPL * d contiguous bytes.  The grid runs over row ranges: wave w
// of block b takes the groups of SQ_T * RPL consecutive rows number (4 b + w), then every (4 gridDim)-th.  A pass carries NQ = 1, 2
// or 4 queries: the rows are loaded once and every query runs its own chain over them (a subtraction and an fma per element and
// query).  The bound is HBM: N d 4 bytes a pass, what wise_ip_topk_f32 reads.  No packed f32 math.
#include "range_common.h"
#include "sq_codec.h"

namespace wise {
namespace l2 {

using namespace ivf_sq;

constexpr int MAX_D = 1024;
constexpr int MAX_NQP = 4;                // queries a pass of the exact scan carries at most

static bool shape_ok(int d) { return d >= 16 && d <= MAX_D && d % 16 == 0; }

// the place of a lane in a wave-load: chunk c of row `sub` of the load; lanes past RPL * C idle
struct LanePlace {
    int C, RPL, sub, c;
    bool active;
    __device__ __forceinline__ void init(int d, int lane) {
        C = d >> 4; RPL = 64 / C; sub = lane / C; c = lane - sub * C; active = sub < RPL;
    }
};

// WHICH ROW an item of a scan stands for
//   ROWS_ALL     item i is row i
//   ROWS_POS     item i is row pos[i] (int64, ascending: wise_l2_topk_pos_f32)
//   ROWS_CAND    item i is row cand[i] (uint32, any order: the candidates of the batched search)
//   ROWS_SAMPLE  item i is row (i / 32) * gstride * 32 + i % 32: evenly spaced groups of 32 rows (the batched search's sample)
enum : int { ROWS_ALL = 0, ROWS_POS = 1, ROWS_CAND = 2, ROWS_SAMPLE = 3 };
struct RowSource {
    const long long* pos;
    const unsigned* cand;
    long long gstride;
};
template <int MODE>
__device__ __forceinline__ long long row_of(const RowSource& src, long long i) {
    if constexpr (MODE == ROWS_POS) return src.pos[i];
    if constexpr (MODE == ROWS_CAND) return (long long)src.cand[i];
    if constexpr (MODE == ROWS_SAMPLE) return (i >> 5) * src.gstride * 32 + (i & 31);
    return i;
}

// One wave's share of a scan over n items: the groups of SQ_T wave-loads number g0, g0 + gstep, ... (in wave-loads).  Every
// distance is sq_score_loads_nq's; a key carries the ROW, so ties go to the lower position whatever the order of the items.
template <int NQ, int MODE>
__device__ __forceinline__ void scan_items(const unsigned char* __restrict__ rows, int d, long long n, long long g0, long long gstep,
                                           const RowSource& src, const LanePlace& L, const float4 (&w)[NQ][4],
                                           WaveList (&wl)[NQ], int lane) {
    const long long ngroups = (n + L.RPL - 1) / L.RPL;
    for (long long g = g0; g < ngroups; g += gstep) {                               // wave-uniform
        long long r[SQ_T];
        bool live[SQ_T];
#pragma unroll
        for (int t = 0; t < SQ_T; ++t) {
            const long long item = (g + t) * L.RPL + L.sub;
            live[t] = L.active && item < n;
            r[t] = row_of<MODE>(src, item < n ? item : n - 1);                      // stay inside the items; masked by live
        }
        float s[NQ][SQ_T];
        sq_score_loads_nq<CodecL2, NQ>(rows, d, L.C, L.c, r, w, s);
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int t = 0; t < SQ_T; ++t) {
                const u64 key = make_key(-s[q][t], (unsigned)r[t]);
                wl[q].offer(live[t] && L.c == 0 && key > wl[q].tau, key, lane);
            }
    }
}

// fold the four wave lists of a block into wave 0's (every wave calls; wave 0 ends with its list sorted, k keys or fewer)
template <int NQ>
__device__ __forceinline__ void fold_block_lists(WaveList (&wl)[NQ], const u64* lds, int cap, int k, int lane, int wave) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) wl[q].compact(lane);
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        for (int w = 1; w < 4; ++w) {
            const u64* other = lds + (size_t)(w * NQ + q) * cap;
            for (int i0 = 0; i0 < k; i0 += 64) {
                const int i = i0 + lane;
                const u64 key = i < k ? other[i] : 0;
                wl[q].offer(key != 0 && key > wl[q].tau, key, lane);
            }
        }
        wl[q].compact(lane);
    }
}

// THE EXACT SCAN.  grid = blocks over row ranges; part [grid][NQ][k] keys for merge_keys_kernel.  gate: the launch does nothing
// unless *gate != 0 (the batched search's fallback)
template <int NQ, int MODE>
__global__ __launch_bounds__(256) void l2_flat_scan_kernel(const unsigned char* __restrict__ rows, long long n, int d,
                                                           const float* __restrict__ Q, int k, int cap, u64* __restrict__ part,
                                                           RowSource src, const int* __restrict__ gate) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (gate && *gate == 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64* lds = reinterpret_cast<u64*>(smem);
    LanePlace L;
    L.init(d, lane);
    float4 w[NQ][4];
#pragma unroll
    for (int q = 0; q < NQ; ++q) CodecL2::weights(Q + (size_t)q * d, d, L.c, w[q]);
    WaveList wl[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) wl[q].init(lds + (size_t)(wave * NQ + q) * cap, cap, k, lane);
    scan_items<NQ, MODE>(rows, d, n, ((long long)blockIdx.x * 4 + wave) * SQ_T, (long long)gridDim.x * 4 * SQ_T, src, L, w, wl, lane);
    fold_block_lists<NQ>(wl, lds, cap, k, lane, wave);
    if (wave == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            u64* dst = part + ((size_t)blockIdx.x * NQ + q) * k;
            for (int i = lane; i < k; i += 64) dst[i] = wl[q].buf[i];
        }
    }
}

// behind the merge: the scores of n outputs become distances again (exact; the padding becomes +3.4028235e38)
__global__ __launch_bounds__(256) void l2_flip_kernel(float* __restrict__ D, int n, const int* __restrict__ gate) {
    if (gate && *gate == 0) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) D[i] = -D[i];
}

// ---- range_search (wise_l2_range_*): ip_sq16.hip's pair over CodecL2; structure, workspace and the determinism argument:
// range_common.h.  A segment is RANGE_ROWS consecutive rows.
// count: block (x, y) owns segment x for the queries y NQ .. y NQ + NQ - 1 (a ragged tile repeats the last query, unwritten)
template <int NQ>
__global__ __launch_bounds__(256) void l2_range_count_kernel(const unsigned char* __restrict__ rows, long long N, int d,
                                                             const float* __restrict__ Q, int nq, float radius,
                                                             const unsigned* __restrict__ keep, unsigned* __restrict__ hit,
                                                             long long wstride, long long* __restrict__ seg, long long ns) {
    __shared__ unsigned hb[NQ][RANGE_WORDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q0 = blockIdx.y * NQ;
    LanePlace L;
    L.init(d, lane);
    float4 w[NQ][4];
#pragma unroll
    for (int q = 0; q < NQ; ++q) CodecL2::weights(Q + (size_t)(q0 + q < nq ? q0 + q : nq - 1) * d, d, L.c, w[q]);
    for (int i = threadIdx.x; i < NQ * RANGE_WORDS; i += 256) hb[i / RANGE_WORDS][i % RANGE_WORDS] = 0u;
    __syncthreads();
    const long long clo = (long long)blockIdx.x * RANGE_ROWS;
    const long long chi = clo + RANGE_ROWS < N ? clo + RANGE_ROWS : N;
    const int ngroups = (int)((chi - clo + L.RPL - 1) / L.RPL);
    for (int g = wave * SQ_T; g < ngroups; g += 4 * SQ_T) {                         // wave-uniform
        long long r[SQ_T];
        bool live[SQ_T];
        bool any = false;
#pragma unroll
        for (int t = 0; t < SQ_T; ++t) {
            r[t] = clo + (long long)(g + t) * L.RPL + L.sub;
            live[t] = L.active && r[t] < chi;
            if (r[t] >= chi) r[t] = chi - 1;                                        // stay inside the segment; masked by live
            if (keep) live[t] = live[t] && ((keep[r[t] >> 5] >> (r[t] & 31)) & 1u) != 0;
            any = any || live[t];
        }
        if (keep && __ballot(any) == 0) continue;
        float s[NQ][SQ_T];
        sq_score_loads_nq<CodecL2, NQ>(rows, d, L.C, L.c, r, w, s);
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int t = 0; t < SQ_T; ++t)
                if (live[t] && L.c == 0 && s[q][t] < radius) range_mark(hb[q], (int)(r[t] - clo));
    }
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

// fill: grid (ns, nq); the hits of one segment, in ascending position, behind lims[q] + the segment's offset
__global__ __launch_bounds__(256) void l2_range_fill_kernel(const unsigned char* __restrict__ rows, long long N, int d,
                                                            const float* __restrict__ Q, const long long* __restrict__ ids,
                                                            long long id_base, const unsigned* __restrict__ hit, long long wstride,
                                                            const long long* __restrict__ seg, long long ns,
                                                            const long long* __restrict__ lims, float* __restrict__ outD,
                                                            long long* __restrict__ outI) {
    __shared__ unsigned short lst[RANGE_ROWS];
    __shared__ int s_cnt;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qi = blockIdx.y, si = blockIdx.x;
    const long long* so = seg + (size_t)qi * (ns + 1) + si;
    const long long left = so[1] - so[0];                        // hits count found in this segment: never more are written
    if (left <= 0) return;                                                         // no hit in this segment (block-uniform)
    const long long dest = lims[qi] + so[0];
    const long long clo = (long long)si * RANGE_ROWS;
    const long long chi = clo + RANGE_ROWS < N ? clo + RANGE_ROWS : N;
    const unsigned* words = hit + (size_t)qi * wstride + (size_t)si * RANGE_WORDS;
    LanePlace L;
    L.init(d, lane);
    float4 w[4];
    CodecL2::weights(Q + (size_t)qi * d, d, L.c, w);
    if (wave == 0) {
        const int n = range_list(words, (int)((chi - clo + 31) >> 5), lst, lane);
        if (lane == 0) s_cnt = n;
    }
    __syncthreads();
    const int cnt = s_cnt < left ? s_cnt : (int)left;
    if (cnt <= 0) return;                                                           // block-uniform
    const int ngroups = (cnt + L.RPL - 1) / L.RPL;
    for (int g = wave * SQ_T; g < ngroups; g += 4 * SQ_T) {
        long long r[SQ_T];
        int e[SQ_T];
#pragma unroll
        for (int t = 0; t < SQ_T; ++t) {
            e[t] = (g + t) * L.RPL + L.sub;
            if (!L.active || e[t] >= cnt) e[t] = -1;
            r[t] = clo + lst[e[t] >= 0 ? e[t] : cnt - 1];
        }
        float s[SQ_T];
        sq_score_loads<CodecL2>(rows, d, L.C, L.c, r, w, s);
#pragma unroll
        for (int t = 0; t < SQ_T; ++t)
            if (e[t] >= 0 && L.c == 0) {
                outD[dest + e[t]] = s[t];
                outI[dest + e[t]] = ids ? ids[r[t]] : id_base + r[t];
            }
    }
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

// ---- the batched search (wise_l2_topk_batched): ip_sq16.hip's threshold form for distances.  With qb = bf16(q) and xb the bf16
// rows, |q - x|^2 / 2 = |q|^2 / 2 + |x|^2 / 2 - q . x, and a(r) = half[r] - (qb . xb_r on the matrix cores) approximates
// (dist(q, r) - |q|^2) / 2 within eps (restated at l2_stage_kernel).  One pass answers up to QB queries:
//   stage    the queries rounded to bf16 (ONE piece), |q|^2 and eps per query; a query whose bf16 image or whose eps is not finite
//            hands the pass to the exact scan at once
//   sample   per query the exact scan's k smallest distances over S0 evenly spaced rows: t = the k-th is an upper bound of the
//            index's exact k-th, so every row of the exact top-k has a(r) <= thr = (t - |q|^2) / 2 + eps
//   collect  every (query, row) with a(r) <= thr[query] is appended to the query's list (any order: the re-scoring keys carry the
//            row); further sample rounds over growing shares of the rows tighten thr first, so that the round over all rows
//            collects a few hundred rows a query
//   rescore  the exact scan's distance of every listed row (scan_items over the list), the k best; a list that overflowed raises
//            the pass's flag instead: every later launch of the pass returns at once and the exact scan queued behind, gated on
//            the flag, answers the pass's queries
constexpr int L2B_CAP = 4096;             // rows a query's candidate list holds
constexpr int L2B_SAMPLE = 8192;          // rows of the first sample
constexpr int L2B_MAX_K = 128;
constexpr long long L2B_MIN_ROWS = 4096;
constexpr int L2B_WAVES = 8;              // waves of a collect block

struct BatchSlots {                       // workspace of a pass
    bf16_t* qb;                           // [QB][d]
    float* eps;                           // [QB]
    float* q2;                            // [QB] |q|^2 (fp32)
    float* thr;                           // [QB]
    int* ctl;                             // [QB] entries offered to a query's list
    int* flag;                            // [1] != 0: a list overflowed or a query has no usable band; the exact scan answers the pass
    unsigned* cand;                       // [QB][L2B_CAP]
};

__device__ __forceinline__ bool is_finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// block = one wave = one query.  eps bounds |a(r) - (dist(q, r) - |q|^2) / 2| plus what the threshold's own arithmetic loses, for
// EVERY row, from norms[0] = M = max |x| and norms[1] = Rx = max |x - xb| alone (u = 2^-24):
//   |q - qb| M                      the query's rounding (Cauchy-Schwarz)
//   |qb| Rx                         the rows' rounding
//   d 2^-22 |q| (M + Rx)            fp32 accumulation of the matrix-core sum (as IndexSQfp16 bounds it)
//   d u M^2 / 2                     the rounding of half[r]: 4 d / 256 <= 16 fmaf and 6 adds of non-negative terms, halved exactly
//   (d + 2) u (|q| + M)^2           the contract distance against the real one; the band needs half of it, the other half pays for
//                                   the rounding of |q|^2 (a sum like half[r]'s), of half[r] - acc and of the threshold's three
//                                   operations, each a few u of at most (|q| + M)^2
//   sqrt(d) (|q| + M) 2^-125 + 1e-33  operands or partial results below the normal range, flushed or not
// every factor is an fp32 result itself and is rounded up by 1.001.
__global__ __launch_bounds__(64) void l2_stage_kernel(const float* __restrict__ Q, int d, const float* __restrict__ norms, BatchSlots ws) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, q = blockIdx.x;
    float e2 = 0.f, q2 = 0.f, b2 = 0.f;
    bool bad = false;
    for (int i = lane; i < d; i += 64) {
        const float v = Q[(size_t)q * d + i];
        const bf16_t h = f32_to_bf16(v);
        ws.qb[(size_t)q * d + i] = h;
        const float back = bf16_to_f32(h), r = v - back;
        bad = bad || !is_finite_f32(back);                        // the bf16 image is infinite or NaN
        e2 = fmaf(r, r, e2);
        q2 = fmaf(v, v, q2);
        b2 = fmaf(back, back, b2);
    }
    e2 = wave_sum(e2);
    q2 = wave_sum(q2);
    b2 = wave_sum(b2);
    const bool any_bad = __ballot(bad) != 0;
    if (lane == 0) {
        const float u = 5.9604644775390625e-08f, fd = (float)d;
        const float M = norms[0] * 1.001f, Rx = norms[1] * 1.001f;
        const float nq = sqrtf(q2) * 1.001f, ne = sqrtf(e2) * 1.001f, nb = sqrtf(b2) * 1.001f;
        const float reach = nq + M;
        float eps = ne * M;
        eps = eps + nb * Rx;
        eps = eps + fd * 4.f * u * nq * (M + Rx);
        eps = eps + fd * u * 0.5f * M * M;
        eps = eps + (fd + 2.f) * u * reach * reach;
        eps = eps + sqrtf(fd) * reach * 2.35098870164457501594e-38f + 1e-33f;
        eps = eps * 1.001f;
        // A query whose bf16 image is not finite, or whose band is not (|q| or M beyond ~1e19), has no usable matrix-core score:
        // it raises the pass's flag here — the host cleared it before this launch — and the exact scan answers the pass.  Every
        // block that raises it stores the same value.
        if (any_bad || !is_finite_f32(eps) || !is_finite_f32(q2)) {
            eps = __builtin_inff();
            *ws.flag = 1;
        }
        ws.eps[q] = eps;
        ws.q2[q] = q2;
        ws.thr[q] = __builtin_inff();
        ws.ctl[q] = 0;
    }
}

// thr of a query whose k-th smallest exact distance over some of the rows is t: (t - |q|^2) / 2 + eps, rounded up
__device__ __forceinline__ float threshold_above(float t, float q2, float eps) {
#pragma clang fp contract(off)
    return ((0.5f * t - 0.5f * q2) + eps) + (t + q2) * 2.384185791015625e-07f + 1e-37f;
}

// block = one query.  ROWS_SAMPLE: the exact top-k over n_sample evenly spaced rows sets thr.  ROWS_CAND: the exact top-k over the
// query's list; final == 0 tightens thr and empties the list, final != 0 writes the answer
template <int MODE>
__global__ __launch_bounds__(256) void l2_query_block_kernel(const unsigned char* __restrict__ rows, int d, const float* __restrict__ Q,
                                                             int k, int cap, long long n_sample, long long gstride, BatchSlots ws,
                                                             int final, const long long* __restrict__ ids, long long id_base,
                                                             float* __restrict__ outD, long long* __restrict__ outI) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = blockIdx.x;
    __shared__ long long s_n;                                                       // items to scan, -1: nothing to do
    if (threadIdx.x == 0) {
        long long n = n_sample;
        if (*ws.flag != 0) {
            n = -1;
        } else if (MODE == ROWS_CAND) {
            n = ws.ctl[q];
            if (n > L2B_CAP) { *ws.flag = 1; n = -1; }
        }
        s_n = n;
    }
    __syncthreads();
    const long long n = s_n;
    if (n < 0) return;                                                              // block-uniform
    // (a block that read flag == 0 goes on although another raises it meanwhile: what it writes is then written again by the
    // exact scan)
    u64* lds = reinterpret_cast<u64*>(smem);
    LanePlace L;
    L.init(d, lane);
    float4 w[1][4];
    CodecL2::weights(Q + (size_t)q * d, d, L.c, w[0]);
    WaveList wl[1];
    wl[0].init(lds + (size_t)wave * cap, cap, k, lane);
    RowSource src{nullptr, ws.cand + (size_t)q * L2B_CAP, gstride};
    scan_items<1, MODE>(rows, d, n, (long long)wave * SQ_T, 4 * SQ_T, src, L, w, wl, lane);
    fold_block_lists<1>(wl, lds, cap, k, lane, wave);
    if (wave != 0) return;
    if (!final) {
        if (lane == 0) {
            const u64 kth = wl[0].buf[k - 1];
            float thr = MODE == ROWS_CAND ? ws.thr[q] : __builtin_inff();
            if (kth != 0) {
                const float t = threshold_above(-f32_unorder((unsigned)(kth >> 32)), ws.q2[q], ws.eps[q]);
                thr = t < thr ? t : thr;
            }
            ws.thr[q] = thr;
            ws.ctl[q] = 0;
        }
        return;
    }
    for (int i = lane; i < k; i += 64) {
        const u64 key = wl[0].buf[i];
        float dist = 3.4028234663852886e38f;
        long long id = -1;
        if (key != 0) {
            const unsigned row = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
            dist = -f32_unorder((unsigned)(key >> 32));
            id = ids ? ids[row] : id_base + (long long)row;
        }
        outD[(size_t)q * k + i] = dist;
        outI[(size_t)q * k + i] = id;
    }
}

// THE COLLECT PASS: sq16_collect_kernel (ip_sq16.hip) over the bf16 rows.  A wave owns groups of 32 rows; lane (i, h) =
// (lane & 31, lane >> 5) streams the 16-byte pieces h C .. h C + C - 1 of row i of Xb — its own half of the row, d contiguous
// bytes — and every piece is the A operand of one v_mfma_f32_32x32x16_bf16 as loaded; the B operand is the same piece of the
// query's bf16 image in LDS (rows of 2 d + 16 bytes: the 16 lanes of a quarter-wave read 16 different 16-byte bank groups).  The
// instruction's k index thereby runs over the pieces in the order (j, C + j) — the order of a sum does not matter to a candidate
// score.  QT = query tiles of 32 a pass carries.  group g stands for rows g * gstride * 32 ..: gstride > 1 is a sample round
// (whole groups only), 1 the round over all rows.  A lane holds 16 rows of its group for 32 QT queries: it reads their half-norms
// (four runs of four consecutive floats) and lists row r for query q iff !(half[r] - acc > thr[q]).
template <int QT>
__global__ __launch_bounds__(L2B_WAVES * 64) void l2_collect_kernel(const bf16_t* __restrict__ rows, const float* __restrict__ half,
                                                                    long long N, int d, int nq, long long ngroups, long long gstride,
                                                                    BatchSlots ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (*ws.flag != 0) return;                                                      // before any barrier
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int ldb = 2 * d + 16, P = d >> 3, C = d >> 4;
    for (int idx = threadIdx.x; idx < QT * 32 * P; idx += L2B_WAVES * 64) {
        const int j = idx / P, p = idx - j * P;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (j < nq) v = reinterpret_cast<const u32x4*>(ws.qb)[(size_t)j * P + p];
        *reinterpret_cast<u32x4*>(smem + (size_t)j * ldb + (size_t)p * 16) = v;
    }
    __syncthreads();
    float thr[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) thr[t] = t * 32 + i < nq ? ws.thr[t * 32 + i] : -__builtin_inff();
    const unsigned char* qbase = smem + (size_t)i * ldb + (size_t)h * C * 16;
    for (long long g = (long long)blockIdx.x * L2B_WAVES + wave; g < ngroups; g += (long long)gridDim.x * L2B_WAVES) {
        const long long row0 = g * gstride * 32;
        const long long mine = row0 + i < N ? row0 + i : N - 1;                     // stay in bounds; masked below
        const bf16x8* src = reinterpret_cast<const bf16x8*>(rows + (size_t)mine * d) + (size_t)h * C;
        f32x16 acc[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        for (int j0 = 0; j0 < C; j0 += 8) {                                         // C % 8 == 0 (d % 128 == 0: host check)
            bf16x8 x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = __builtin_nontemporal_load(src + j0 + j);
            // the eight loads of a lane — one 128-byte line — go out back to back (see sq16_collect_kernel)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int t = 0; t < QT; ++t) {
                    const bf16x8 b = *reinterpret_cast<const bf16x8*>(qbase + (size_t)t * 32 * ldb + (size_t)(j0 + j) * 16);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[j], b, acc[t], 0, 0, 0);
                }
        }
        // acc[t][r]: row (r & 3) + 8 (r >> 2) + 4 h of the group, query 32 t + i
        float hv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long row = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            hv[r] = half[row < N ? row : N - 1];                                    // stay in bounds; masked below
        }
        bool hit = false;
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) hit |= !(hv[r] - acc[t][r] > thr[t]);
        if (__ballot(hit) == 0) continue;
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long row = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const int q = t * 32 + i;
                if (row < N && q < nq && !(hv[r] - acc[t][r] > thr[t])) {   // a NaN score is a candidate, never a silent loss
                    const int at = atomicAdd(ws.ctl + q, 1);
                    if (at < L2B_CAP) ws.cand[(size_t)q * L2B_CAP + at] = (unsigned)row;
                }
            }
    }
}

// the end of a pass: who answered its nq queries
__global__ void l2_pass_counters_kernel(const int* __restrict__ flag, int nq, int* __restrict__ counters) {
    if (threadIdx.x == 0 && blockIdx.x == 0) atomicAdd(counters + (*flag != 0 ? 1 : 0), nq);
}

// ---- host side
struct L2Plan {
    int cap, grid;
    size_t lds;
};
// geometry of one launch of the exact scan carrying nqp queries over n items
static L2Plan plan_l2(long long n, int d, int nqp, int k) {
    L2Plan p;
    p.cap = topk_list_cap(k);
    p.lds = (size_t)4 * nqp * p.cap * 8;
    const int blocks_per_cu = p.lds > 80 * 1024 ? 1 : p.lds > 40 * 1024 ? 2 : 4;
    p.grid = 256 * blocks_per_cu;
    const int rpl = 64 / (d >> 4);
    const long long loads = (n + rpl - 1) / rpl;
    long long need = (loads + 4 * SQ_T - 1) / (4 * SQ_T);
    if (need < 1) need = 1;
    if (p.grid > need) p.grid = (int)need;
    return p;
}
// queries a pass may carry: LDS (4 waves * nqp lists <= 64 KiB, so that two blocks fit a CU) — the rule of plan_scan (ip_topk.hip)
static int l2_queries_per_pass(int nq, int k) {
    const int cap = topk_list_cap(k);
    int nqp = 1;
    while (nqp * 2 <= nq && nqp * 2 <= MAX_NQP && (size_t)4 * nqp * 2 * cap * 8 <= 64 * 1024) nqp <<= 1;
    return nqp;
}
static size_t l2_part_bytes(long long n, int d, int nq, int k) {
    size_t keys = 0;
    for (int nqp = l2_queries_per_pass(nq, k); nqp >= 1; nqp >>= 1) {
        const size_t v = (size_t)plan_l2(n, d, nqp, k).grid * nqp * k;
        if (v > keys) keys = v;
    }
    return align_up(keys * sizeof(u64), 256);
}

template <int NQ, int MODE>
static void launch_flat_scan(const L2Plan& p, const unsigned char* rows, long long n, int d, const float* Q, int k, u64* part,
                             const RowSource& src, const int* gate, hipStream_t st) {
    auto kern = l2_flat_scan_kernel<NQ, MODE>;
    if (p.lds > 48 * 1024) raise_lds_limit(reinterpret_cast<const void*>(kern), (int)p.lds);
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(256), p.lds, st, rows, n, d, Q, k, p.cap, part, src, gate);
}

// the exact scan, its merge and the flip for nq queries over n items (pos == nullptr: the rows 0 .. n - 1), up to MAX_NQP queries
// a pass: a pass carries the largest power of two of queries that is left.  workspace: l2_part_bytes(n, d, nq, k)
static int l2_topk(const void* rows, long long n, int d, const float* Q, int nq, int k, const int64_t* ids, int64_t id_base,
                   float* outD, int64_t* outI, void* workspace, hipStream_t st, const long long* pos, const int* gate) {
    const unsigned char* rb = reinterpret_cast<const unsigned char*>(rows);
    u64* part = reinterpret_cast<u64*>(workspace);
    const int nqp_max = l2_queries_per_pass(nq, k);
    const RowSource src{pos, nullptr, 1};
    for (int q0 = 0; q0 < nq;) {
        int nqp = nqp_max;
        while (nqp > nq - q0) nqp >>= 1;
        const L2Plan p = plan_l2(n, d, nqp, k);
        const float* qp = Q + (size_t)q0 * d;
        if (n > 0) {
            ProfScope prof(PROF_SCAN, (double)n * d * 4.0, st);
            if (pos) {
                if (nqp == 4) launch_flat_scan<4, ROWS_POS>(p, rb, n, d, qp, k, part, src, gate, st);
                else if (nqp == 2) launch_flat_scan<2, ROWS_POS>(p, rb, n, d, qp, k, part, src, gate, st);
                else launch_flat_scan<1, ROWS_POS>(p, rb, n, d, qp, k, part, src, gate, st);
            } else {
                if (nqp == 4) launch_flat_scan<4, ROWS_ALL>(p, rb, n, d, qp, k, part, src, gate, st);
                else if (nqp == 2) launch_flat_scan<2, ROWS_ALL>(p, rb, n, d, qp, k, part, src, gate, st);
                else launch_flat_scan<1, ROWS_ALL>(p, rb, n, d, qp, k, part, src, gate, st);
            }
            WISE_LAUNCH_CHECK("l2_flat_scan_kernel");
        }
        if (int rc = launch_merge_keys(part, n > 0 ? p.grid : 0, nqp, nqp, k, reinterpret_cast<const long long*>(ids), (long long)id_base,
                                       outD, reinterpret_cast<long long*>(outI), q0, st, gate))
            return rc;
        const int cells = nqp * k;
        hipLaunchKernelGGL(l2_flip_kernel, dim3((cells + 255) / 256), dim3(256), 0, st, outD + (size_t)q0 * k, cells, gate);
        WISE_LAUNCH_CHECK("l2_flip_kernel");
        q0 += nqp;
    }
    return WISE_OK;
}

static int topk_args(const char* what, const void* rows, int64_t N, int d, const float* Q, int nq, int k, const float* outD,
                     const int64_t* outI) {
    WISE_CHECK_ARG(shape_ok(d), "%s: d=%d unsupported (d %% 16 == 0 in [16, 1024])", what, d);
    WISE_CHECK_ARG(k >= 1 && k <= 2048, "%s: k=%d out of [1,2048]", what, k);
    WISE_CHECK_ARG(nq >= 1 && nq <= 1024, "%s: nq=%d out of [1,1024]", what, nq);
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll, "%s: N=%lld out of range", what, (long long)N);
    WISE_CHECK_ARG(Q && outD && outI && (rows || N == 0), "%s: null pointer", what);
    WISE_CHECK_ARG(((uintptr_t)rows & 15) == 0 && ((uintptr_t)Q & 15) == 0, "%s: rows and Q must be 16-byte aligned", what);
    return WISE_OK;
}

// queries a batched pass carries: their bf16 images (rows of 2 d + 16 bytes) must fit LDS (160 KiB)
static int batch_pass_queries(int d) { return d <= 512 ? 128 : 64; }
static bool batch_shape_ok(int64_t N, int d, int nq, int k) {
    return d >= 256 && d <= MAX_D && d % 128 == 0 && nq >= 3 && nq <= 1024 && k >= 1 && k <= L2B_MAX_K && N >= L2B_MIN_ROWS &&
           N < (1ll << 31);
}
static size_t batch_slot_bytes(int d, BatchSlots* ws, unsigned char* base) {
    const int qb = batch_pass_queries(d);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        unsigned char* p = base ? base + off : nullptr;
        off += align_up(bytes, 256);
        return p;
    };
    unsigned char* qimg = take((size_t)qb * d * 2);
    unsigned char* eps = take((size_t)qb * 4);
    unsigned char* q2 = take((size_t)qb * 4);
    unsigned char* thr = take((size_t)qb * 4);
    unsigned char* ctl = take((size_t)qb * 4);
    unsigned char* flag = take(4);
    unsigned char* cand = take((size_t)qb * L2B_CAP * 4);
    if (ws) {
        ws->qb = reinterpret_cast<bf16_t*>(qimg);
        ws->eps = reinterpret_cast<float*>(eps);
        ws->q2 = reinterpret_cast<float*>(q2);
        ws->thr = reinterpret_cast<float*>(thr);
        ws->ctl = reinterpret_cast<int*>(ctl);
        ws->flag = reinterpret_cast<int*>(flag);
        ws->cand = reinterpret_cast<unsigned*>(cand);
    }
    return off;
}

template <int QT>
static void launch_collect(const bf16_t* rows, const float* half, long long N, int d, int nq, long long ngroups, long long gstride,
                           const BatchSlots& ws, hipStream_t st) {
    const size_t lds = (size_t)QT * 32 * (2 * d + 16);
    auto kern = l2_collect_kernel<QT>;
    if (lds > 48 * 1024) raise_lds_limit(reinterpret_cast<const void*>(kern), (int)lds);
    long long grid = (ngroups + L2B_WAVES - 1) / L2B_WAVES;
    const long long most = 256 * (lds > 80 * 1024 ? 1 : 2);
    if (grid > most) grid = most;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(L2B_WAVES * 64), lds, st, rows, half, N, d, nq, ngroups, gstride, ws);
}

template <int MODE>
static void launch_query_blocks(const void* rows, int d, const float* Q, int nq, int k, long long n_sample, long long gstride,
                                const BatchSlots& ws, int final, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI,
                                hipStream_t st) {
    const int cap = topk_list_cap(k);
    hipLaunchKernelGGL(l2_query_block_kernel<MODE>, dim3(nq), dim3(256), (size_t)4 * cap * 8, st,
                       reinterpret_cast<const unsigned char*>(rows), d, Q, k, cap, n_sample, gstride, ws, final,
                       reinterpret_cast<const long long*>(ids), (long long)id_base, outD, reinterpret_cast<long long*>(outI));
}

}  // namespace l2
}  // namespace wise

using namespace wise;
using namespace wise::l2;

extern "C" size_t wise_l2_topk_workspace_bytes(int64_t N, int d, int nq, int k) {
    if (N < 0 || N >= 0xFFFFFFFFll || !shape_ok(d) || nq < 1 || nq > 1024 || k < 1 || k > 2048) return 0;
    return l2_part_bytes(N, d, nq, k) + 256;
}

extern "C" int wise_l2_topk_f32(const float* X, int64_t N, int d, const float* Q, int nq, int k, const int64_t* ids, int64_t id_base,
                                float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = topk_args("l2_topk_f32", X, N, d, Q, nq, k, outD, outI)) return rc;
    const size_t need = wise_l2_topk_workspace_bytes(N, d, nq, k);
    WISE_CHECK_ARG(workspace && workspace_bytes >= need, "l2_topk_f32: workspace %zu < %zu bytes", workspace_bytes, need);
    return l2_topk(X, N, d, Q, nq, k, ids, id_base, outD, outI, workspace, (hipStream_t)stream, nullptr, nullptr);
}

extern "C" int wise_l2_topk_pos_f32(const float* X, int64_t N, int d, const int64_t* pos, int64_t n_pos, const float* Q, int nq, int k,
                                    const int64_t* ids, int64_t id_base, float* outD, int64_t* outI, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    if (int rc = topk_args("l2_topk_pos_f32", X, N, d, Q, nq, k, outD, outI)) return rc;
    WISE_CHECK_ARG(n_pos >= 0 && n_pos <= N && (pos || n_pos == 0), "l2_topk_pos_f32: n_pos=%lld out of [0, N=%lld] or null positions",
                   (long long)n_pos, (long long)N);
    const size_t need = wise_l2_topk_workspace_bytes(n_pos, d, nq, k);
    WISE_CHECK_ARG(workspace && workspace_bytes >= need, "l2_topk_pos_f32: workspace %zu < %zu bytes", workspace_bytes, need);
    return l2_topk(X, n_pos, d, Q, nq, k, ids, id_base, outD, outI, workspace, (hipStream_t)stream,
                   n_pos > 0 ? reinterpret_cast<const long long*>(pos) : nullptr, nullptr);
}

static bool l2_range_shape_ok(int64_t N, int d, int nq) { return N >= 0 && N < 0xFFFFFFFFll && shape_ok(d) && nq >= 1 && nq <= 65535; }

extern "C" size_t wise_l2_range_workspace_bytes(int64_t N, int d, int nq) {
    if (!l2_range_shape_ok(N, d, nq)) return 0;
    const long long ns = range_flat_segments(N);
    return range_workspace_bytes(nq, ns * RANGE_WORDS, ns);
}

static int l2_range_args(const char* what, const void* rows, int64_t N, int d, const float* Q, int nq, float radius, void* workspace,
                         size_t workspace_bytes) {
    WISE_CHECK_ARG(shape_ok(d), "%s: d=%d unsupported (d %% 16 == 0 in [16, 1024])", what, d);
    WISE_CHECK_ARG(l2_range_shape_ok(N, d, nq), "%s: N=%lld nq=%d out of range (nq <= 65535)", what, (long long)N, nq);
    WISE_CHECK_ARG(Q && (rows || N == 0), "%s: null pointer", what);
    WISE_CHECK_ARG(((uintptr_t)rows & 15) == 0 && ((uintptr_t)Q & 15) == 0, "%s: rows and Q must be 16-byte aligned", what);
    WISE_CHECK_ARG(radius == radius && radius - radius == 0.f, "%s: radius must be finite", what);
    const size_t need = wise_l2_range_workspace_bytes(N, d, nq);
    WISE_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace %zu < %zu bytes", what, workspace_bytes, need);
    return WISE_OK;
}

extern "C" int wise_l2_range_count_f32(const float* X, int64_t N, int d, const float* Q, int nq, float radius, const uint32_t* keep,
                                       int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = l2_range_args("l2_range_count_f32", X, N, d, Q, nq, radius, workspace, workspace_bytes)) return rc;
    WISE_CHECK_ARG(counts, "l2_range_count_f32: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const long long ns = range_flat_segments(N), wstride = ns * RANGE_WORDS;
    unsigned* hit = reinterpret_cast<unsigned*>(workspace);
    long long* seg = reinterpret_cast<long long*>(reinterpret_cast<unsigned char*>(workspace) + range_hit_bytes(nq, wstride));
    const unsigned char* rb = reinterpret_cast<const unsigned char*>(X);
    if (ns > 0) {
        const int nqp = nq >= 4 ? 4 : nq >= 2 ? 2 : 1;
        const dim3 grid((unsigned)ns, (unsigned)((nq + nqp - 1) / nqp));
        ProfScope prof(PROF_SCAN, (double)N * d * 4.0 * grid.y, st);
        if (nqp == 4)
            hipLaunchKernelGGL(l2_range_count_kernel<4>, grid, dim3(256), 0, st, rb, (long long)N, d, Q, nq, radius, keep, hit, wstride, seg, ns);
        else if (nqp == 2)
            hipLaunchKernelGGL(l2_range_count_kernel<2>, grid, dim3(256), 0, st, rb, (long long)N, d, Q, nq, radius, keep, hit, wstride, seg, ns);
        else
            hipLaunchKernelGGL(l2_range_count_kernel<1>, grid, dim3(256), 0, st, rb, (long long)N, d, Q, nq, radius, keep, hit, wstride, seg, ns);
        WISE_LAUNCH_CHECK("l2_range_count_kernel");
    }
    hipLaunchKernelGGL(range_scan_kernel, dim3(nq), dim3(1024), 0, st, seg, ns, reinterpret_cast<long long*>(counts));
    WISE_LAUNCH_CHECK("range_scan_kernel");
    return WISE_OK;
}

extern "C" int wise_l2_range_fill_f32(const float* X, int64_t N, int d, const float* Q, int nq, float radius, const int64_t* ids,
                                      int64_t id_base, const int64_t* lims, float* outD, int64_t* outI, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    if (int rc = l2_range_args("l2_range_fill_f32", X, N, d, Q, nq, radius, workspace, workspace_bytes)) return rc;
    WISE_CHECK_ARG(lims && outD && outI, "l2_range_fill_f32: null pointer");
    const long long ns = range_flat_segments(N), wstride = ns * RANGE_WORDS;
    if (ns == 0) return WISE_OK;
    const unsigned* hit = reinterpret_cast<const unsigned*>(workspace);
    const long long* seg = reinterpret_cast<const long long*>(reinterpret_cast<unsigned char*>(workspace) + range_hit_bytes(nq, wstride));
    hipLaunchKernelGGL(l2_range_fill_kernel, dim3((unsigned)ns, (unsigned)nq), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned char*>(X), (long long)N, d, Q, reinterpret_cast<const long long*>(ids),
                       (long long)id_base, hit, wstride, seg, ns, reinterpret_cast<const long long*>(lims), outD,
                       reinterpret_cast<long long*>(outI));
    WISE_LAUNCH_CHECK("l2_range_fill_kernel");
    return WISE_OK;
}

extern "C" int wise_l2_prepare(const float* X, int64_t N, int d, uint16_t* Xb, float* half, float* norms, void* stream) {
    WISE_CHECK_ARG(shape_ok(d), "l2_prepare: d=%d unsupported (d %% 16 == 0 in [16, 1024])", d);
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll && norms && ((X && Xb && half) || N == 0), "l2_prepare: bad argument");
    WISE_CHECK_ARG(((uintptr_t)X & 15) == 0 && ((uintptr_t)Xb & 15) == 0, "l2_prepare: X and Xb must be 16-byte aligned");
    if (int rc = wise_ip_shadow_bf16(X, N, d, Xb, norms, stream)) return rc;        // the copy and the two norms
    if (N == 0) return WISE_OK;
    long long grid = (N + 3) / 4;
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(l2_half_norm_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, X, (long long)N, d, half);
    WISE_LAUNCH_CHECK("l2_half_norm_kernel");
    return WISE_OK;
}

extern "C" size_t wise_l2_topk_batched_workspace_bytes(int64_t N, int d, int nq, int k) {
    if (!batch_shape_ok(N, d, nq, k)) return 0;
    const int qb = batch_pass_queries(d);
    return batch_slot_bytes(d, nullptr, nullptr) + l2_part_bytes(N, d, nq < qb ? nq : qb, k) + 256;
}

extern "C" int wise_l2_topk_batched(const float* X, const uint16_t* Xb, const float* half, const float* norms, int64_t N, int d,
                                    const float* Q, int nq, int k, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI,
                                    int32_t* counters, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = topk_args("l2_topk_batched", X, N, d, Q, nq, k, outD, outI)) return rc;
    WISE_CHECK_ARG(batch_shape_ok(N, d, nq, k),
                   "l2_topk_batched: N=%lld d=%d nq=%d k=%d not served (d %% 128 == 0 in [256, 1024], nq >= 3, k <= 128, N >= 4096)",
                   (long long)N, d, nq, k);
    WISE_CHECK_ARG(Xb && half && norms, "l2_topk_batched: null pointer");
    WISE_CHECK_ARG(((uintptr_t)Xb & 15) == 0 && ((uintptr_t)half & 3) == 0, "l2_topk_batched: Xb must be 16-byte aligned");
    const size_t need = wise_l2_topk_batched_workspace_bytes(N, d, nq, k);
    WISE_CHECK_ARG(workspace && workspace_bytes >= need, "l2_topk_batched: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    BatchSlots ws;
    unsigned char* wsb = reinterpret_cast<unsigned char*>(workspace);
    void* scan_ws = wsb + batch_slot_bytes(d, &ws, wsb);
    const int qb = batch_pass_queries(d);

    // the rounds of a pass, from the shape alone (wise_ipsq16_topk_batched's rule): a first sample of S0 rows scored exactly, then
    // collect rounds over shares of the rows that grow by the same factor each, at most `ratio` — a round over S' rows under the
    // threshold of a round over S rows lists about k S' / S rows a query, a quarter of what a list holds at
    // ratio = L2B_CAP / (4 k) — and the round over all rows
    const long long full_groups = N / 32;                                           // >= 128
    const long long S0 = (N < L2B_SAMPLE ? N : L2B_SAMPLE) & ~31ll;
    const double ratio = L2B_CAP / (4.0 * k) > 4.0 ? L2B_CAP / (4.0 * k) : 4.0;
    int rounds = 1;                                                                 // collect rounds, the last over all rows
    {
        double reach = (double)S0 * ratio;
        while (reach < (double)N) { reach *= ratio; ++rounds; }
    }
    const double per = pow((double)N / (double)S0, 1.0 / rounds);

    for (int q0 = 0; q0 < nq; q0 += qb) {
        const int nqa = nq - q0 < qb ? nq - q0 : qb;
        const float* Qp = Q + (size_t)q0 * d;
        float* oD = outD + (size_t)q0 * k;
        int64_t* oI = outI + (size_t)q0 * k;
        {
            const hipError_t e = hipMemsetAsync(ws.flag, 0, sizeof(int), st);      // the pass's flag: the stage kernel may raise it
            if (e != hipSuccess) { set_error("l2_topk_batched: memset: %s", hipGetErrorString(e)); return (int)e; }
        }
        hipLaunchKernelGGL(l2_stage_kernel, dim3(nqa), dim3(64), 0, st, Qp, d, norms, ws);
        WISE_LAUNCH_CHECK("l2_stage_kernel");
        launch_query_blocks<ROWS_SAMPLE>(X, d, Qp, nqa, k, S0, full_groups / (S0 / 32), ws, 0, nullptr, 0, nullptr, nullptr, st);
        WISE_LAUNCH_CHECK("l2_query_block_kernel<sample>");
        const int qt = nqa > 64 ? 4 : nqa > 32 ? 2 : 1;
        for (int r = 1; r <= rounds; ++r) {
            const bool last = r == rounds;
            long long groups = (N + 31) / 32, gstride = 1;
            if (!last) {
                groups = (long long)((double)S0 * pow(per, (double)r)) / 32;
                if (groups > full_groups) groups = full_groups;
                if (groups < 1) groups = 1;
                gstride = full_groups / groups;
            }
            {
                ProfScope prof(PROF_SCAN, (double)groups * 32 * d * 2.0, st);
                if (qt == 4) launch_collect<4>(Xb, half, N, d, nqa, groups, gstride, ws, st);
                else if (qt == 2) launch_collect<2>(Xb, half, N, d, nqa, groups, gstride, ws, st);
                else launch_collect<1>(Xb, half, N, d, nqa, groups, gstride, ws, st);
            }
            WISE_LAUNCH_CHECK("l2_collect_kernel");
            launch_query_blocks<ROWS_CAND>(X, d, Qp, nqa, k, 0, 1, ws, last ? 1 : 0, ids, id_base, oD, oI, st);
            WISE_LAUNCH_CHECK("l2_query_block_kernel<cand>");
        }
        if (counters) {
            hipLaunchKernelGGL(l2_pass_counters_kernel, dim3(1), dim3(64), 0, st, ws.flag, nqa, counters);
            WISE_LAUNCH_CHECK("l2_pass_counters_kernel");
        }
        // the exact scan, gated on the flag: returns at once unless a list overflowed
        if (int rc = l2_topk(X, N, d, Qp, nqa, k, ids, id_base, oD, oI, scan_ws, st, nullptr, ws.flag)) return rc;
    }
    return WISE_OK;
}

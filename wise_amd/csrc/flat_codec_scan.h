// The flat codec scans: everything IndexSQfp16 (ip_sq16.hip), IndexFlatL2 (l2_topk.hip), IndexSQ8bit (ip_sq8.hip) and IndexSQfp16L2
// (l2_sq16.hip) share, written once and templated on a METRIC POLICY M.  The four files keep their policy, the kernels that belong
// to one type alone (the inner-product stage kernels with their error bands, reconstruct, the norm kernels, the flip) and their
// extern "C" entry points, which are thin calls into the drivers below.  `static` on what is no template: four translation units
// include this header and each gets its own copy.
// WHAT LIVES HERE: the exact scan (flat_scan_kernel, flat_topk, topk_entry), the range pair (flat_range_*_kernel, range_count,
// range_fill), the batched search (flat_query_block_kernel, flat_collect_kernel, topk_batched), their workspace planners and
// argument checks (topk_args, range_args, batched_args), and the pieces two types share: the sum of squares of a binary16 row
// (square_halves, half_row_square_sum), the grid of the wave-per-row kernels (wave_row_grid), and the stage kernel and threshold of
// the two squared-L2 types (l2_stage_kernel<Image, ROW_TERM>, threshold_above).  The id lookup of the reconstruct kernels is
// row_of_id (topk_common.h); f16x8 stands beside bf16x8 (common.h).
//
// HOW A WAVE-LOAD IS LAID OUT.  A row is C = d / 16 chunks; lane (sub, c) of a wave-load holds chunk c of row sub, RPL = 64 / C
// whole rows per load and SQ_T loads in flight.  Chunk c is the row's 16-byte pieces c, C + c, ... (Codec::PIECES of them: two
// for binary16 rows, four for fp32 rows), so each of a wave-load's load instructions reads RPL * d contiguous bytes.  The grid
// runs over row ranges: wave w of block b takes the groups of SQ_T * RPL consecutive rows number (4 b + w), then every
// (4 gridDim)-th.  A pass carries NQ = 1, 2 or 4 queries: the rows are loaded once and every query runs its own chain over them
// (sq_score_loads_nq of sq_codec.h; for binary16 rows 1 v_fma_mix_f32 per element and query: at 4 queries 2 VALU lane-operations
// per byte, 32 B / clock / CU where HBM delivers about 13).  The bound is HBM: N * Codec::row_bytes(d) a pass.  Selection is the
// flat scan's: sortable (score, position) keys, per-wave threshold lists, merge_keys_kernel (ip_topk.hip).  No packed f32 math.
//
// THE POLICY: plain static members, no virtuals, nothing decided at run time.
//   Codec                      Codec16, CodecL2, Codec8 or Codec16L2 (sq_codec.h): the loads, the weights and the chain of a row's sum s
//   base(b, q), score(s, b)    the per-query base term (b: the array the entry point hands over, q: the query of the pass) and the
//                              row's score as the caller sees it.  PlainPolicy: no base, score = s, nothing is loaded; IndexSQ8bit
//                              (ip_sq8.hip): b[q] = q0 of wise_sq_query and score = q0 + s, ONE fp32 addition.  Keys, the range test
//                              and every returned value are on score
//   key_score(sc)              what the keys order, larger is better: sc, or -sc for a distance (negating an fp32 value is exact)
//   out_score(ks)              a key's score as the caller sees it: the inverse of key_score
//   PAD                        the output score of a slot that no row fills (-3.4028235e38, +3.4028235e38 for a distance)
//   FLIP                       launch_merge_keys writes key scores: a pass of M::flip over its output follows
//   range_hit(s, radius)       the range test: s > radius, s < radius for a distance
//   thr_open(), thr_shut()     the collect thresholds that list every row (before the first sample) and no row (query slots past nq)
//   tighten(thr, t, ws, q)     the threshold after a round whose k-th exact output score was t: never looser than thr
//   Piece, mfma(a, b, acc)     the 8-element operand of the collect pass and its v_mfma_f32_32x32x16_* instruction
//   LOAD_PIECES, operand(x, p) operands a 16-byte load of the collect pass holds: 1 (16-bit rows: the load IS the operand), or 2 (8-bit
//                              codes: operand p = the load's codes 8 p .. 8 p + 7 expanded in registers)
//   QUERY_EXP                  BatchSlots carries a per-query power of two (the stage kernel's scaling of the query image)
//   HALF_NORMS                 the collect score is half[row] - acc, not acc: the half-norms are loaded, and BatchSlots carries |q|^2
//   candidate(hv, acc, thr)    the collect test, written so that a NaN score is a candidate
//   stage(...)                 launches the type's stage kernel (query images, eps, the opening thresholds); returns its name
#pragma once
#include "range_common.h"
#include "sq_codec.h"

namespace wise {
namespace flat_codec {

using namespace ivf_sq;

constexpr int MAX_D = 1024;
constexpr int MAX_NQP = 4;                // queries a pass of the exact scan carries at most

// what a policy over 16-bit collect rows whose score is the row's sum itself inherits
struct PlainPolicy {
    static constexpr int LOAD_PIECES = 1;
    static constexpr bool QUERY_EXP = false;
    static __device__ __forceinline__ float base(const float*, int) { return 0.f; }
    static __device__ __forceinline__ float score(float s, float) { return s; }
};

static bool shape_ok(int d) { return d >= 16 && d <= MAX_D && d % 16 == 0; }

// blocks of a kernel whose waves take one row at a time, four waves a block (the norm and half-norm kernels of the prepare entry points)
static unsigned wave_row_grid(int64_t N) { return (unsigned)((N + 3) / 4 < 2048 ? (N + 3) / 4 : 2048); }

// THE SUM OF SQUARES OF A BINARY16 ROW (wise_ipsq16_prepare, wise_l2sq16_prepare), one wave per row: lane l runs s = fmaf(x, x, s)
// over the widened elements of the row's 16-byte pieces (8 halves each) l, l + 64 in ascending order from +0, and the lanes are
// folded by wave_sum's butterfly (lane masks 32, 16, 8, 4, 2, 1): a row's sum depends on the row alone.
__device__ __forceinline__ float square_halves(float s, unsigned word) {
    const f16x2 h = __builtin_bit_cast(f16x2, word);
    const float a = (float)h.x, b = (float)h.y;
    s = fmaf(a, a, s);
    return fmaf(b, b, s);
}
__device__ __forceinline__ float half_row_square_sum(const unsigned char* __restrict__ rows, long long r, int d, int lane) {
    const u32x4* src = reinterpret_cast<const u32x4*>(rows + (size_t)r * 2 * d);
    float s = 0.f;
    for (int p = lane; p < (d >> 3); p += 64) {
        const u32x4 x = src[p];
        s = square_halves(s, x[0]);
        s = square_halves(s, x[1]);
        s = square_halves(s, x[2]);
        s = square_halves(s, x[3]);
    }
    return wave_sum(s);
}

// the place of a lane in a wave-load (sq_scan_list's): chunk c of row `sub` of the load; lanes past RPL * C idle
struct LanePlace {
    int C, RPL, sub, c;
    bool active;
    __device__ __forceinline__ void init(int d, int lane) {
        C = d >> 4; RPL = 64 / C; sub = lane / C; c = lane - sub * C; active = sub < RPL;
    }
};

// WHICH ROW an item of a scan stands for
//   ROWS_ALL     item i is row i
//   ROWS_POS     item i is row pos[i] (int64, ascending: the *_topk_pos entry points)
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
// score is sq_score_loads_nq's; a key carries the ROW, so ties go to the lower position whatever the order of the items.
template <class M, int NQ, int MODE>
__device__ __forceinline__ void scan_items(const unsigned char* __restrict__ rows, int d, long long n, long long g0, long long gstep,
                                           const RowSource& src, const LanePlace& L, const float4 (&w)[NQ][4], const float (&qb)[NQ],
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
        sq_score_loads_nq<typename M::Codec, NQ>(rows, d, L.C, L.c, r, w, s);
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int t = 0; t < SQ_T; ++t) {
                const u64 key = make_key(M::key_score(M::score(s[q][t], qb[q])), (unsigned)r[t]);
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
template <class M, int NQ, int MODE>
__global__ __launch_bounds__(256) void flat_scan_kernel(const unsigned char* __restrict__ rows, long long n, int d,
                                                        const float* __restrict__ Q, const float* __restrict__ base, int k, int cap,
                                                        u64* __restrict__ part, RowSource src, const int* __restrict__ gate) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (gate && *gate == 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64* lds = reinterpret_cast<u64*>(smem);
    LanePlace L;
    L.init(d, lane);
    float4 w[NQ][4];
#pragma unroll
    for (int q = 0; q < NQ; ++q) M::Codec::weights(Q + (size_t)q * d, d, L.c, w[q]);
    float qb[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) qb[q] = M::base(base, q);
    WaveList wl[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) wl[q].init(lds + (size_t)(wave * NQ + q) * cap, cap, k, lane);
    scan_items<M, NQ, MODE>(rows, d, n, ((long long)blockIdx.x * 4 + wave) * SQ_T, (long long)gridDim.x * 4 * SQ_T, src, L, w, qb, wl, lane);
    fold_block_lists<NQ>(wl, lds, cap, k, lane, wave);
    if (wave == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            u64* dst = part + ((size_t)blockIdx.x * NQ + q) * k;
            for (int i = lane; i < k; i += 64) dst[i] = wl[q].buf[i];
        }
    }
}

// ---- range_search: the flat form of sq_range_count_kernel / sq_range_fill_kernel (ivf_sq.hip); structure, workspace and the
// determinism argument: range_common.h.  A segment is RANGE_ROWS consecutive rows.
// count: block (x, y) owns segment x for the queries y NQ .. y NQ + NQ - 1 (a ragged tile repeats the last query, unwritten)
template <class M, int NQ>
__global__ __launch_bounds__(256) void flat_range_count_kernel(const unsigned char* __restrict__ rows, long long N, int d,
                                                               const float* __restrict__ Q, const float* __restrict__ base, int nq,
                                                               float radius, const unsigned* __restrict__ keep, unsigned* __restrict__ hit,
                                                               long long wstride, long long* __restrict__ seg, long long ns) {
    __shared__ unsigned hb[NQ][RANGE_WORDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q0 = blockIdx.y * NQ;
    LanePlace L;
    L.init(d, lane);
    float4 w[NQ][4];
#pragma unroll
    for (int q = 0; q < NQ; ++q) M::Codec::weights(Q + (size_t)(q0 + q < nq ? q0 + q : nq - 1) * d, d, L.c, w[q]);
    float qb[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) qb[q] = M::base(base, q0 + q < nq ? q0 + q : nq - 1);
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
        sq_score_loads_nq<typename M::Codec, NQ>(rows, d, L.C, L.c, r, w, s);
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int t = 0; t < SQ_T; ++t)
                if (live[t] && L.c == 0 && M::range_hit(M::score(s[q][t], qb[q]), radius)) range_mark(hb[q], (int)(r[t] - clo));
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

// ---- search_grouped, stage 1 (group_topk.hip holds stages 2 and 3): flat_range_count_kernel with the hit mark replaced by one store.
// Block (x, y) owns segment x for the queries y NQ .. y NQ + NQ - 1 and leaves, per query, ord[q][r] = f32_order(key score of row r)
// — the upper half of the key the exact scan makes of that (query, row) — for every row r of the segment; a row cleared in keep
// reads 0, the keys' empty value.  The images are gathered in LDS and leave as whole runs of 4-byte words: every row of the
// segment is written, selected or not, so nothing has to be cleared first.
template <class M, int NQ>
__global__ __launch_bounds__(256) void flat_group_scores_kernel(const unsigned char* __restrict__ rows, long long N, int d,
                                                                const float* __restrict__ Q, const float* __restrict__ base, int nq,
                                                                const unsigned* __restrict__ keep, unsigned* __restrict__ ord) {
    __shared__ unsigned sc[NQ][RANGE_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q0 = blockIdx.y * NQ;
    LanePlace L;
    L.init(d, lane);
    float4 w[NQ][4];
#pragma unroll
    for (int q = 0; q < NQ; ++q) M::Codec::weights(Q + (size_t)(q0 + q < nq ? q0 + q : nq - 1) * d, d, L.c, w[q]);
    float qb[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) qb[q] = M::base(base, q0 + q < nq ? q0 + q : nq - 1);
    for (int i = threadIdx.x; i < NQ * RANGE_ROWS; i += 256) sc[i / RANGE_ROWS][i % RANGE_ROWS] = 0u;
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
        sq_score_loads_nq<typename M::Codec, NQ>(rows, d, L.C, L.c, r, w, s);
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int t = 0; t < SQ_T; ++t)
                if (live[t] && L.c == 0) sc[q][(int)(r[t] - clo)] = f32_order(M::key_score(M::score(s[q][t], qb[q])));
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        if (q0 + q >= nq) break;
        unsigned* dst = ord + (size_t)(q0 + q) * (size_t)N + (size_t)clo;
        for (int i = threadIdx.x; i < (int)(chi - clo); i += 256) dst[i] = sc[q][i];
    }
}

// fill: grid (ns, nq); the hits of one segment, in ascending position, behind lims[q] + the segment's offset
template <class M>
__global__ __launch_bounds__(256) void flat_range_fill_kernel(const unsigned char* __restrict__ rows, long long N, int d,
                                                              const float* __restrict__ Q, const float* __restrict__ base,
                                                              const long long* __restrict__ ids, long long id_base,
                                                              const unsigned* __restrict__ hit, long long wstride,
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
    M::Codec::weights(Q + (size_t)qi * d, d, L.c, w);
    const float qb = M::base(base, qi);
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
        sq_score_loads<typename M::Codec>(rows, d, L.C, L.c, r, w, s);
#pragma unroll
        for (int t = 0; t < SQ_T; ++t)
            if (e[t] >= 0 && L.c == 0) {
                outD[dest + e[t]] = M::score(s[t], qb);
                outI[dest + e[t]] = ids ? ids[r[t]] : id_base + r[t];
            }
    }
}

// ---- the batched search.  One pass answers up to QB queries (in the words of a score; a distance turns every sense round):
//   stage    M::stage: the queries rounded to ONE 16-bit piece and, per query, eps = the bound on |collect score - what the exact
//            scan's score implies| of any row (restated at each stage kernel); a query without a usable image
//            or band hands the pass to the exact scan at once
//   sample   per query the exact scan's top-k over S0 evenly spaced rows: t = the k-th score bounds the index's exact k-th from
//            the loose side, so every row of the exact top-k passes the threshold M::tighten makes of t and eps
//   collect  every (query, row) whose matrix-core score passes thr[query] is appended to the query's list (any order: the
//            re-scoring keys carry the row); further sample rounds over growing shares of the rows tighten thr first, so that the
//            round over all rows collects a few hundred rows a query
//   rescore  the exact scan's score of every listed row (scan_items over the list), the k best; a list that overflowed raises the
//            pass's flag instead: every later launch of the pass returns at once and the exact scan queued behind, gated on the
//            flag, answers the pass's queries
constexpr int BATCH_CAP = 4096;           // rows a query's candidate list holds
constexpr int BATCH_SAMPLE = 8192;        // rows of the first sample
constexpr int BATCH_MAX_K = 128;
constexpr long long BATCH_MIN_ROWS = 4096;
constexpr int BATCH_WAVES = 8;            // waves of a collect block

struct BatchSlots {                       // workspace of a pass
    union {                               // [QB][d] the queries' 16-bit image, under the name each stage kernel writes it by
        _Float16* q16;                    //   binary16 (IndexSQfp16)
        bf16_t* qb;                       //   bf16 (IndexFlatL2)
    };
    float* eps;                           // [QB]
    float* q2;                            // [QB] |q|^2 (fp32); carved for M::HALF_NORMS only
    float* thr;                           // [QB]
    int* qexp;                            // [QB] the power of two the stage kernel scaled the query image by; carved for M::QUERY_EXP only
    const float* base;                    // [nq of the pass] the queries' base terms (M::base), the entry point's array; not carved
    int* ctl;                             // [QB] entries offered to a query's list
    int* flag;                            // [1] != 0: a list overflowed or a query has no usable image or band; the exact scan answers the pass
    unsigned* cand;                       // [QB][BATCH_CAP]
};

__device__ __forceinline__ bool is_finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// ---- the stage kernel and the threshold of the two squared-L2 types (IndexFlatL2: bf16 image, rows with a rounding term;
// IndexSQfp16L2: binary16 image, rows used as stored).  With q16 the query's 16-bit image and x16 the 16-bit rows,
// |q - x|^2 / 2 = |q|^2 / 2 + |x|^2 / 2 - q . x, and a(r) = half[r] - (q16 . x16_r on the matrix cores) approximates
// (dist(q, r) - |q|^2) / 2 within eps:
//   stage    the queries rounded to the image (ONE piece), |q|^2 and eps per query; a query whose image or whose eps is not finite
//            hands the pass to the exact scan at once
//   sample   t = the k-th smallest distance over the sample is an upper bound of the index's exact k-th, so every row of the exact
//            top-k has a(r) <= thr = (t - |q|^2) / 2 + eps
//   collect  every (query, row) with a(r) <= thr[query] is listed
// a query element rounded into the image; returns the image's value
__device__ __forceinline__ float round_image(bf16_t* dst, float v) {
    const bf16_t h = f32_to_bf16(v);
    *dst = h;
    return bf16_to_f32(h);
}
__device__ __forceinline__ float round_image(_Float16* dst, float v) {
    const _Float16 h = (_Float16)v;
    *dst = h;
    return (float)h;
}

// block = one wave = one query.  eps bounds |a(r) - (dist(q, r) - |q|^2) / 2| plus what the threshold's own arithmetic loses, for
// EVERY row, from norms[0] = M = max |x| and, under ROW_TERM, norms[1] = Rx = max |x - x16| alone (u = 2^-24):
//   |q - q16| M                     the query's rounding (Cauchy-Schwarz)
//   |q16| Rx                        the rows' rounding                                    (ROW_TERM only: binary16 rows drop it)
//   d 2^-22 |q| (M + Rx)            fp32 accumulation of the matrix-core sum (as IndexSQfp16 bounds it; binary16 rows: Rx = 0)
//   d u M^2 / 2                     the rounding of half[r]: at most 16 fmaf and 6 adds of non-negative terms, halved exactly
//   (d + 2) u (|q| + M)^2           the contract distance against the real one; the band needs half of it, the other half pays for
//                                   the rounding of |q|^2 (a sum like half[r]'s), of half[r] - acc and of the threshold's three
//                                   operations, each a few u of at most (|q| + M)^2
//   sqrt(d) (|q| + M) 2^-125 + 1e-33  operands or partial results below the normal range, flushed or not
// every factor is an fp32 result itself and is rounded up by 1.001.
template <class Image, bool ROW_TERM>
__global__ __launch_bounds__(64) void l2_stage_kernel(const float* __restrict__ Q, int d, const float* __restrict__ norms, BatchSlots ws) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, q = blockIdx.x;
    Image* image = reinterpret_cast<Image*>(ws.qb);
    float e2 = 0.f, q2 = 0.f, b2 = 0.f;
    bool bad = false;
    for (int i = lane; i < d; i += 64) {
        const float v = Q[(size_t)q * d + i];
        const float back = round_image(image + (size_t)q * d + i, v), r = v - back;
        bad = bad || !is_finite_f32(back);                        // the image is infinite or NaN
        e2 = fmaf(r, r, e2);
        q2 = fmaf(v, v, q2);
        if constexpr (ROW_TERM) b2 = fmaf(back, back, b2);
    }
    e2 = wave_sum(e2);
    q2 = wave_sum(q2);
    if constexpr (ROW_TERM) b2 = wave_sum(b2);
    const bool any_bad = __ballot(bad) != 0;
    if (lane == 0) {
        const float u = 5.9604644775390625e-08f, fd = (float)d;
        const float M = norms[0] * 1.001f;
        const float nq = sqrtf(q2) * 1.001f, ne = sqrtf(e2) * 1.001f;
        const float reach = nq + M;
        float eps = ne * M;
        if constexpr (ROW_TERM) {
            const float Rx = norms[1] * 1.001f, nb = sqrtf(b2) * 1.001f;
            eps = eps + nb * Rx;
            eps = eps + fd * 4.f * u * nq * (M + Rx);
        } else {
            eps = eps + fd * 4.f * u * nq * M;
        }
        eps = eps + fd * u * 0.5f * M * M;
        eps = eps + (fd + 2.f) * u * reach * reach;
        eps = eps + sqrtf(fd) * reach * 2.35098870164457501594e-38f + 1e-33f;
        eps = eps * 1.001f;
        // A query whose image is not finite (a binary16 component beyond 65504), or whose band is not (|q| or M beyond ~1e19), has
        // no usable matrix-core score: it raises the pass's flag here — the host cleared it before this launch — and the exact scan
        // answers the pass.  Every block that raises it stores the same value.
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
template <class M, int MODE>
__global__ __launch_bounds__(256) void flat_query_block_kernel(const unsigned char* __restrict__ rows, int d, const float* __restrict__ Q,
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
            if (n > BATCH_CAP) { *ws.flag = 1; n = -1; }
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
    M::Codec::weights(Q + (size_t)q * d, d, L.c, w[0]);
    const float qb[1] = {M::base(ws.base, q)};
    WaveList wl[1];
    wl[0].init(lds + (size_t)wave * cap, cap, k, lane);
    RowSource src{nullptr, ws.cand + (size_t)q * BATCH_CAP, gstride};
    scan_items<M, 1, MODE>(rows, d, n, (long long)wave * SQ_T, 4 * SQ_T, src, L, w, qb, wl, lane);
    fold_block_lists<1>(wl, lds, cap, k, lane, wave);
    if (wave != 0) return;
    if (!final) {
        if (lane == 0) {
            const u64 kth = wl[0].buf[k - 1];
            float thr = MODE == ROWS_CAND ? ws.thr[q] : M::thr_open();
            if (kth != 0) thr = M::tighten(thr, M::out_score(f32_unorder((unsigned)(kth >> 32))), ws, q);
            ws.thr[q] = thr;
            ws.ctl[q] = 0;
        }
        return;
    }
    for (int i = lane; i < k; i += 64) {
        const u64 key = wl[0].buf[i];
        float dscore = M::PAD;
        long long id = -1;
        if (key != 0) {
            const unsigned row = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
            dscore = M::out_score(f32_unorder((unsigned)(key >> 32)));
            id = ids ? ids[row] : id_base + (long long)row;
        }
        outD[(size_t)q * k + i] = dscore;
        outI[(size_t)q * k + i] = id;
    }
}

// THE COLLECT PASS over the 16-bit rows (the binary16 rows themselves, or the bf16 copy of fp32 rows).  A wave owns groups of
// 32 rows; lane (i, h) = (lane & 31, lane >> 5) streams the 16-byte pieces h C .. h C + C - 1 of row i — its own half of the row,
// d contiguous bytes — and every piece is the A operand of one M::mfma as loaded; the B operand is the same piece of the query's
// 16-bit image in LDS (rows of 2 d + 16 bytes: the 16 lanes of a quarter-wave read 16 different 16-byte bank groups).  The
// instruction's k index thereby runs over the pieces in the order (j, C + j) — the order of a sum does not matter to a candidate
// score.  QT = query tiles of 32 a pass carries.  group g stands for rows g * gstride * 32 ..: gstride > 1 is a sample round
// (whole groups only), 1 the round over all rows.  A lane holds 16 rows of its group for 32 QT queries; under M::HALF_NORMS it
// reads their half-norms (four runs of four consecutive floats).  Row r is listed for query q iff M::candidate.
// 8-BIT CODES (M::LOAD_PIECES == 2: IndexSQ8bit).  A row is d bytes; the lane's half of it is d / 32 loads of 16 codes, and a load is
// expanded in registers to the TWO operands of its codes 0 .. 7 and 8 .. 15 (M::operand), each against the matching piece of the
// query image; the loads go out four at a time — the same eight MFMAs per query tile between two bursts of loads.
template <class M, int QT>
__global__ __launch_bounds__(BATCH_WAVES * 64) void flat_collect_kernel(const unsigned char* __restrict__ rows, const float* __restrict__ half,
                                                                        long long N, int d, int nq, long long ngroups,
                                                                        long long gstride, BatchSlots ws) {
    using Piece = typename M::Piece;
    constexpr int LP = M::LOAD_PIECES, NL = 8 / LP;                                 // operands a load holds, loads of a burst
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (*ws.flag != 0) return;                                                      // before any barrier
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int ldb = 2 * d + 16, P = d >> 3, C = d / (16 * LP);                      // C: loads of a lane's half row
    for (int idx = threadIdx.x; idx < QT * 32 * P; idx += BATCH_WAVES * 64) {
        const int j = idx / P, p = idx - j * P;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (j < nq) v = reinterpret_cast<const u32x4*>(ws.qb)[(size_t)j * P + p];
        *reinterpret_cast<u32x4*>(smem + (size_t)j * ldb + (size_t)p * 16) = v;
    }
    __syncthreads();
    float thr[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) thr[t] = t * 32 + i < nq ? ws.thr[t * 32 + i] : M::thr_shut();
    const unsigned char* qbase = smem + (size_t)i * ldb + (size_t)h * d;           // the image of the lane's half row: d bytes in
    for (long long g = (long long)blockIdx.x * BATCH_WAVES + wave; g < ngroups; g += (long long)gridDim.x * BATCH_WAVES) {
        const long long row0 = g * gstride * 32;
        const long long mine = row0 + i < N ? row0 + i : N - 1;                     // stay in bounds; masked below
        const u32x4* src = reinterpret_cast<const u32x4*>(rows + (size_t)mine * (size_t)(2 * d / LP)) + (size_t)h * C;
        f32x16 acc[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        for (int j0 = 0; j0 < C; j0 += NL) {                                        // C % NL == 0 (d % 128 == 0: host check)
            u32x4 x[NL];
#pragma unroll
            for (int j = 0; j < NL; ++j) x[j] = __builtin_nontemporal_load(src + j0 + j);
            // the loads of a lane's burst — one 128-byte line of 16-bit rows — go out back to back: spread between the MFMAs, as
            // the scheduler would have them, a line is evicted from the vector cache between its pieces and fetched again for each
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < NL; ++j)
#pragma unroll
                for (int p = 0; p < LP; ++p) {
                    Piece a;
                    if constexpr (LP == 1) a = __builtin_bit_cast(Piece, x[j]);
                    else a = M::operand(x[j], p);
#pragma unroll
                    for (int t = 0; t < QT; ++t) {
                        const Piece b = *reinterpret_cast<const Piece*>(qbase + (size_t)t * 32 * ldb + (size_t)((j0 + j) * LP + p) * 16);
                        acc[t] = M::mfma(a, b, acc[t]);
                    }
                }
        }
        // acc[t][r]: row (r & 3) + 8 (r >> 2) + 4 h of the group, query 32 t + i
        float hv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if constexpr (M::HALF_NORMS) {
                const long long row = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                hv[r] = half[row < N ? row : N - 1];                                // stay in bounds; masked below
            } else {
                hv[r] = 0.f;                                                        // (no load is issued; M::candidate ignores it)
            }
        }
        bool hit = false;
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) hit |= M::candidate(hv[r], acc[t][r], thr[t]);
        if (__ballot(hit) == 0) continue;
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long row = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const int q = t * 32 + i;
                if (row < N && q < nq && M::candidate(hv[r], acc[t][r], thr[t])) {  // a NaN score is a candidate, never a silent loss
                    const int at = atomicAdd(ws.ctl + q, 1);
                    if (at < BATCH_CAP) ws.cand[(size_t)q * BATCH_CAP + at] = (unsigned)row;
                }
            }
    }
}

// the end of a pass: who answered its nq queries
static __global__ void flat_pass_counters_kernel(const int* __restrict__ flag, int nq, int* __restrict__ counters) {
    if (threadIdx.x == 0 && blockIdx.x == 0) atomicAdd(counters + (*flag != 0 ? 1 : 0), nq);
}

// ---- host side
struct FlatPlan {
    int cap, grid;
    size_t lds;
};
// geometry of one launch of the exact scan carrying nqp queries over n items
static FlatPlan plan_flat(long long n, int d, int nqp, int k) {
    FlatPlan p;
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
static int queries_per_pass(int nq, int k) {
    const int cap = topk_list_cap(k);
    int nqp = 1;
    while (nqp * 2 <= nq && nqp * 2 <= MAX_NQP && (size_t)4 * nqp * 2 * cap * 8 <= 64 * 1024) nqp <<= 1;
    return nqp;
}
static size_t part_bytes(long long n, int d, int nq, int k) {
    size_t keys = 0;
    for (int nqp = queries_per_pass(nq, k); nqp >= 1; nqp >>= 1) {
        const size_t v = (size_t)plan_flat(n, d, nqp, k).grid * nqp * k;
        if (v > keys) keys = v;
    }
    return align_up(keys * sizeof(u64), 256);
}

template <class M, int NQ, int MODE>
static void launch_flat_scan(const FlatPlan& p, const unsigned char* rows, long long n, int d, const float* Q, const float* base, int k,
                             u64* part, const RowSource& src, const int* gate, hipStream_t st) {
    auto kern = flat_scan_kernel<M, NQ, MODE>;
    if (p.lds > 48 * 1024) raise_lds_limit(reinterpret_cast<const void*>(kern), (int)p.lds);
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(256), p.lds, st, rows, n, d, Q, base, k, p.cap, part, src, gate);
}

// the exact scan, its merge (and the flip where M::FLIP) for nq queries over n items (pos == nullptr: the rows 0 .. n - 1), up to
// MAX_NQP queries a pass: a pass carries the largest power of two of queries that is left.  base: the queries' base terms (M::base),
// nullptr under a policy that has none.  workspace: part_bytes(n, d, nq, k)
template <class M>
static int flat_topk(const void* rows, long long n, int d, const float* Q, const float* base, int nq, int k, const int64_t* ids, int64_t id_base,
                     float* outD, int64_t* outI, void* workspace, hipStream_t st, const long long* pos, const int* gate) {
    const unsigned char* rb = reinterpret_cast<const unsigned char*>(rows);
    u64* part = reinterpret_cast<u64*>(workspace);
    const int nqp_max = queries_per_pass(nq, k);
    const RowSource src{pos, nullptr, 1};
    for (int q0 = 0; q0 < nq;) {
        int nqp = nqp_max;
        while (nqp > nq - q0) nqp >>= 1;
        const FlatPlan p = plan_flat(n, d, nqp, k);
        const float* qp = Q + (size_t)q0 * d;
        const float* bp = base ? base + q0 : nullptr;
        if (n > 0) {
            ProfScope prof(PROF_SCAN, (double)n * (double)M::Codec::row_bytes(d), st);
            if (pos) {
                if (nqp == 4) launch_flat_scan<M, 4, ROWS_POS>(p, rb, n, d, qp, bp, k, part, src, gate, st);
                else if (nqp == 2) launch_flat_scan<M, 2, ROWS_POS>(p, rb, n, d, qp, bp, k, part, src, gate, st);
                else launch_flat_scan<M, 1, ROWS_POS>(p, rb, n, d, qp, bp, k, part, src, gate, st);
            } else {
                if (nqp == 4) launch_flat_scan<M, 4, ROWS_ALL>(p, rb, n, d, qp, bp, k, part, src, gate, st);
                else if (nqp == 2) launch_flat_scan<M, 2, ROWS_ALL>(p, rb, n, d, qp, bp, k, part, src, gate, st);
                else launch_flat_scan<M, 1, ROWS_ALL>(p, rb, n, d, qp, bp, k, part, src, gate, st);
            }
            WISE_LAUNCH_CHECK("flat_scan_kernel");
        }
        if (int rc = launch_merge_keys(part, n > 0 ? p.grid : 0, nqp, nqp, k, reinterpret_cast<const long long*>(ids), (long long)id_base,
                                       outD, reinterpret_cast<long long*>(outI), q0, st, gate))
            return rc;
        if constexpr (M::FLIP) {
            if (int rc = M::flip(outD + (size_t)q0 * k, nqp * k, gate, st)) return rc;
        }
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

static size_t topk_workspace_bytes(int64_t N, int d, int nq, int k) {
    if (N < 0 || N >= 0xFFFFFFFFll || !shape_ok(d) || nq < 1 || nq > 1024 || k < 1 || k > 2048) return 0;
    return part_bytes(N, d, nq, k) + 256;
}

// the *_topk and *_topk_pos entry points: by_pos scans the n_pos rows pos[] of the N, else all N
template <class M>
static int topk_entry(const char* what, const void* rows, int64_t N, int d, bool by_pos, const int64_t* pos, int64_t n_pos, const float* Q,
                      const float* base, int nq, int k, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI, void* workspace,
                      size_t workspace_bytes, void* stream) {
    if (int rc = topk_args(what, rows, N, d, Q, nq, k, outD, outI)) return rc;
    if (by_pos)
        WISE_CHECK_ARG(n_pos >= 0 && n_pos <= N && (pos || n_pos == 0), "%s: n_pos=%lld out of [0, N=%lld] or null positions", what,
                       (long long)n_pos, (long long)N);
    const int64_t n = by_pos ? n_pos : N;
    const size_t need = topk_workspace_bytes(n, d, nq, k);
    WISE_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace %zu < %zu bytes", what, workspace_bytes, need);
    return flat_topk<M>(rows, n, d, Q, base, nq, k, ids, id_base, outD, outI, workspace, (hipStream_t)stream,
                        by_pos && n_pos > 0 ? reinterpret_cast<const long long*>(pos) : nullptr, nullptr);
}

static bool range_shape_ok(int64_t N, int d, int nq) { return N >= 0 && N < 0xFFFFFFFFll && shape_ok(d) && nq >= 1 && nq <= 65535; }

static size_t range_workspace(int64_t N, int d, int nq) {
    if (!range_shape_ok(N, d, nq)) return 0;
    const long long ns = range_flat_segments(N);
    return range_workspace_bytes(nq, ns * RANGE_WORDS, ns);
}

static int range_args(const char* what, const void* rows, int64_t N, int d, const float* Q, int nq, float radius, void* workspace,
                      size_t workspace_bytes) {
    WISE_CHECK_ARG(shape_ok(d), "%s: d=%d unsupported (d %% 16 == 0 in [16, 1024])", what, d);
    WISE_CHECK_ARG(range_shape_ok(N, d, nq), "%s: N=%lld nq=%d out of range (nq <= 65535)", what, (long long)N, nq);
    WISE_CHECK_ARG(Q && (rows || N == 0), "%s: null pointer", what);
    WISE_CHECK_ARG(((uintptr_t)rows & 15) == 0 && ((uintptr_t)Q & 15) == 0, "%s: rows and Q must be 16-byte aligned", what);
    WISE_CHECK_ARG(radius == radius && radius - radius == 0.f, "%s: radius must be finite", what);
    const size_t need = range_workspace(N, d, nq);
    WISE_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace %zu < %zu bytes", what, workspace_bytes, need);
    return WISE_OK;
}

template <class M>
static int range_count(const char* what, const void* rows, int64_t N, int d, const float* Q, const float* base, int nq, float radius, const uint32_t* keep,
                       int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = range_args(what, rows, N, d, Q, nq, radius, workspace, workspace_bytes)) return rc;
    WISE_CHECK_ARG(counts, "%s: null pointer", what);
    hipStream_t st = (hipStream_t)stream;
    const long long ns = range_flat_segments(N), wstride = ns * RANGE_WORDS;
    unsigned* hit = reinterpret_cast<unsigned*>(workspace);
    long long* seg = reinterpret_cast<long long*>(reinterpret_cast<unsigned char*>(workspace) + range_hit_bytes(nq, wstride));
    const unsigned char* rb = reinterpret_cast<const unsigned char*>(rows);
    if (ns > 0) {
        const int nqp = nq >= 4 ? 4 : nq >= 2 ? 2 : 1;
        const dim3 grid((unsigned)ns, (unsigned)((nq + nqp - 1) / nqp));
        ProfScope prof(PROF_SCAN, (double)N * (double)M::Codec::row_bytes(d) * grid.y, st);
        if (nqp == 4)
            hipLaunchKernelGGL((flat_range_count_kernel<M, 4>), grid, dim3(256), 0, st, rb, (long long)N, d, Q, base, nq, radius, keep, hit, wstride, seg, ns);
        else if (nqp == 2)
            hipLaunchKernelGGL((flat_range_count_kernel<M, 2>), grid, dim3(256), 0, st, rb, (long long)N, d, Q, base, nq, radius, keep, hit, wstride, seg, ns);
        else
            hipLaunchKernelGGL((flat_range_count_kernel<M, 1>), grid, dim3(256), 0, st, rb, (long long)N, d, Q, base, nq, radius, keep, hit, wstride, seg, ns);
        WISE_LAUNCH_CHECK("flat_range_count_kernel");
    }
    hipLaunchKernelGGL(range_scan_kernel, dim3(nq), dim3(1024), 0, st, seg, ns, reinterpret_cast<long long*>(counts));
    WISE_LAUNCH_CHECK("range_scan_kernel");
    return WISE_OK;
}

template <class M>
static int range_fill(const char* what, const void* rows, int64_t N, int d, const float* Q, const float* base, int nq, float radius, const int64_t* ids,
                      int64_t id_base, const int64_t* lims, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes,
                      void* stream) {
    if (int rc = range_args(what, rows, N, d, Q, nq, radius, workspace, workspace_bytes)) return rc;
    WISE_CHECK_ARG(lims && outD && outI, "%s: null pointer", what);
    const long long ns = range_flat_segments(N), wstride = ns * RANGE_WORDS;
    if (ns == 0) return WISE_OK;
    const unsigned* hit = reinterpret_cast<const unsigned*>(workspace);
    const long long* seg = reinterpret_cast<const long long*>(reinterpret_cast<unsigned char*>(workspace) + range_hit_bytes(nq, wstride));
    hipLaunchKernelGGL(flat_range_fill_kernel<M>, dim3((unsigned)ns, (unsigned)nq), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned char*>(rows), (long long)N, d, Q, base, reinterpret_cast<const long long*>(ids),
                       (long long)id_base, hit, wstride, seg, ns, reinterpret_cast<const long long*>(lims), outD,
                       reinterpret_cast<long long*>(outI));
    WISE_LAUNCH_CHECK("flat_range_fill_kernel");
    return WISE_OK;
}

// the *_group_scores entry points: ord [nq][N] receives every row's ordered key score, 0 for the rows keep clears
template <class M>
static int group_scores(const char* what, const void* rows, int64_t N, int d, const float* Q, const float* base, int nq, const uint32_t* keep,
                        uint32_t* ord, void* stream) {
    WISE_CHECK_ARG(shape_ok(d), "%s: d=%d unsupported (d %% 16 == 0 in [16, 1024])", what, d);
    WISE_CHECK_ARG(range_shape_ok(N, d, nq), "%s: N=%lld nq=%d out of range (nq <= 65535)", what, (long long)N, nq);
    WISE_CHECK_ARG(Q && (rows || N == 0) && (ord || N == 0), "%s: null pointer", what);
    WISE_CHECK_ARG(((uintptr_t)rows & 15) == 0 && ((uintptr_t)Q & 15) == 0, "%s: rows and Q must be 16-byte aligned", what);
    const long long ns = range_flat_segments(N);
    if (ns == 0) return WISE_OK;
    hipStream_t st = (hipStream_t)stream;
    const unsigned char* rb = reinterpret_cast<const unsigned char*>(rows);
    const int nqp = nq >= 4 ? 4 : nq >= 2 ? 2 : 1;
    const dim3 grid((unsigned)ns, (unsigned)((nq + nqp - 1) / nqp));
    ProfScope prof(PROF_SCAN, (double)N * (double)M::Codec::row_bytes(d) * grid.y, st);
    if (nqp == 4)
        hipLaunchKernelGGL((flat_group_scores_kernel<M, 4>), grid, dim3(256), 0, st, rb, (long long)N, d, Q, base, nq, keep, ord);
    else if (nqp == 2)
        hipLaunchKernelGGL((flat_group_scores_kernel<M, 2>), grid, dim3(256), 0, st, rb, (long long)N, d, Q, base, nq, keep, ord);
    else
        hipLaunchKernelGGL((flat_group_scores_kernel<M, 1>), grid, dim3(256), 0, st, rb, (long long)N, d, Q, base, nq, keep, ord);
    WISE_LAUNCH_CHECK("flat_group_scores_kernel");
    return WISE_OK;
}

// queries a batched pass carries: their 16-bit images (rows of 2 d + 16 bytes) must fit LDS (160 KiB)
static int batch_pass_queries(int d) { return d <= 512 ? 128 : 64; }
static bool batch_shape_ok(int64_t N, int d, int nq, int k) {
    return d >= 256 && d <= MAX_D && d % 128 == 0 && nq >= 3 && nq <= 1024 && k >= 1 && k <= BATCH_MAX_K && N >= BATCH_MIN_ROWS &&
           N < (1ll << 31);
}
template <class M>
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
    unsigned char* q2 = M::HALF_NORMS ? take((size_t)qb * 4) : nullptr;
    unsigned char* thr = take((size_t)qb * 4);
    unsigned char* qexp = M::QUERY_EXP ? take((size_t)qb * 4) : nullptr;
    unsigned char* ctl = take((size_t)qb * 4);
    unsigned char* flag = take(4);
    unsigned char* cand = take((size_t)qb * BATCH_CAP * 4);
    if (ws) {
        ws->qb = reinterpret_cast<bf16_t*>(qimg);
        ws->eps = reinterpret_cast<float*>(eps);
        ws->q2 = reinterpret_cast<float*>(q2);
        ws->thr = reinterpret_cast<float*>(thr);
        ws->qexp = reinterpret_cast<int*>(qexp);
        ws->base = nullptr;
        ws->ctl = reinterpret_cast<int*>(ctl);
        ws->flag = reinterpret_cast<int*>(flag);
        ws->cand = reinterpret_cast<unsigned*>(cand);
    }
    return off;
}
template <class M>
static size_t batched_workspace_bytes(int64_t N, int d, int nq, int k) {
    if (!batch_shape_ok(N, d, nq, k)) return 0;
    const int qb = batch_pass_queries(d);
    return batch_slot_bytes<M>(d, nullptr, nullptr) + part_bytes(N, d, nq < qb ? nq : qb, k) + 256;
}

// what every *_topk_batched entry point checks before anything of its own; need: its *_topk_batched_workspace_bytes
static int batched_args(const char* what, const void* rows, int64_t N, int d, const float* Q, int nq, int k, const float* outD,
                        const int64_t* outI, const float* norms, const void* workspace, size_t workspace_bytes, size_t need) {
    if (int rc = topk_args(what, rows, N, d, Q, nq, k, outD, outI)) return rc;
    WISE_CHECK_ARG(batch_shape_ok(N, d, nq, k),
                   "%s: N=%lld d=%d nq=%d k=%d not served (d %% 128 == 0 in [256, 1024], nq >= 3, k <= 128, N >= 4096)", what,
                   (long long)N, d, nq, k);
    WISE_CHECK_ARG(norms, "%s: null pointer", what);
    WISE_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace %zu < %zu bytes", what, workspace_bytes, need);
    return WISE_OK;
}

template <class M, int QT>
static void launch_collect(const unsigned char* rows, const float* half, long long N, int d, int nq, long long ngroups, long long gstride,
                           const BatchSlots& ws, hipStream_t st) {
    const size_t lds = (size_t)QT * 32 * (2 * d + 16);
    auto kern = flat_collect_kernel<M, QT>;
    if (lds > 48 * 1024) raise_lds_limit(reinterpret_cast<const void*>(kern), (int)lds);
    long long grid = (ngroups + BATCH_WAVES - 1) / BATCH_WAVES;
    const long long most = 256 * (lds > 80 * 1024 ? 1 : 2);
    if (grid > most) grid = most;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(BATCH_WAVES * 64), lds, st, rows, half, N, d, nq, ngroups, gstride, ws);
}

template <class M, int MODE>
static void launch_query_blocks(const void* rows, int d, const float* Q, int nq, int k, long long n_sample, long long gstride,
                                const BatchSlots& ws, int final, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI,
                                hipStream_t st) {
    const int cap = topk_list_cap(k);
    hipLaunchKernelGGL((flat_query_block_kernel<M, MODE>), dim3(nq), dim3(256), (size_t)4 * cap * 8, st,
                       reinterpret_cast<const unsigned char*>(rows), d, Q, k, cap, n_sample, gstride, ws, final,
                       reinterpret_cast<const long long*>(ids), (long long)id_base, outD, reinterpret_cast<long long*>(outI));
}

// the *_topk_batched entry points behind their argument checks.  rows: what the exact routine scores; rows16 (and half, where
// M::HALF_NORMS): what the collect pass streams — 16-bit rows, or the 8-bit codes themselves (M::LOAD_PIECES == 2).  base: as
// flat_topk.  workspace: batched_workspace_bytes<M>(N, d, nq, k)
template <class M>
static int topk_batched(const char* what, const void* rows, const void* rows16, const float* half, const float* norms, int64_t N, int d,
                        const float* Q, const float* base, int nq, int k, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI,
                        int32_t* counters, void* workspace, hipStream_t st) {
    BatchSlots ws;
    unsigned char* wsb = reinterpret_cast<unsigned char*>(workspace);
    void* scan_ws = wsb + batch_slot_bytes<M>(d, &ws, wsb);
    const int qb = batch_pass_queries(d);
    const unsigned char* crows = reinterpret_cast<const unsigned char*>(rows16);

    // the rounds of a pass, from the shape alone: a first sample of S0 rows scored exactly, then collect rounds over shares of the
    // rows that grow by the same factor each, at most `ratio` — a round over S' rows under the threshold of a round over S rows
    // lists about k S' / S rows a query, a quarter of what a list holds at ratio = BATCH_CAP / (4 k) — and the round over all rows
    const long long full_groups = N / 32;                                           // >= 128
    const long long S0 = (N < BATCH_SAMPLE ? N : BATCH_SAMPLE) & ~31ll;
    const double ratio = BATCH_CAP / (4.0 * k) > 4.0 ? BATCH_CAP / (4.0 * k) : 4.0;
    int rounds = 1;                                                                 // collect rounds, the last over all rows
    {
        double reach = (double)S0 * ratio;
        while (reach < (double)N) { reach *= ratio; ++rounds; }
    }
    const double per = pow((double)N / (double)S0, 1.0 / rounds);

    for (int q0 = 0; q0 < nq; q0 += qb) {
        const int nqa = nq - q0 < qb ? nq - q0 : qb;
        const float* Qp = Q + (size_t)q0 * d;
        const float* bp = base ? base + q0 : nullptr;
        ws.base = bp;
        float* oD = outD + (size_t)q0 * k;
        int64_t* oI = outI + (size_t)q0 * k;
        {
            const hipError_t e = hipMemsetAsync(ws.flag, 0, sizeof(int), st);      // the pass's flag: the stage kernel may raise it
            if (e != hipSuccess) { set_error("%s: memset: %s", what, hipGetErrorString(e)); return (int)e; }
        }
        const char* stage_name = M::stage(Qp, d, norms, ws, nqa, st);
        WISE_LAUNCH_CHECK(stage_name);
        launch_query_blocks<M, ROWS_SAMPLE>(rows, d, Qp, nqa, k, S0, full_groups / (S0 / 32), ws, 0, nullptr, 0, nullptr, nullptr, st);
        WISE_LAUNCH_CHECK("flat_query_block_kernel<sample>");
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
                ProfScope prof(PROF_SCAN, (double)groups * 32 * d * 2.0 / M::LOAD_PIECES, st);
                if (qt == 4) launch_collect<M, 4>(crows, half, N, d, nqa, groups, gstride, ws, st);
                else if (qt == 2) launch_collect<M, 2>(crows, half, N, d, nqa, groups, gstride, ws, st);
                else launch_collect<M, 1>(crows, half, N, d, nqa, groups, gstride, ws, st);
            }
            WISE_LAUNCH_CHECK("flat_collect_kernel");
            launch_query_blocks<M, ROWS_CAND>(rows, d, Qp, nqa, k, 0, 1, ws, last ? 1 : 0, ids, id_base, oD, oI, st);
            WISE_LAUNCH_CHECK("flat_query_block_kernel<cand>");
        }
        if (counters) {
            hipLaunchKernelGGL(flat_pass_counters_kernel, dim3(1), dim3(64), 0, st, ws.flag, nqa, counters);
            WISE_LAUNCH_CHECK("flat_pass_counters_kernel");
        }
        // the exact scan, gated on the flag: returns at once unless a list overflowed
        if (int rc = flat_topk<M>(rows, N, d, Qp, bp, nqa, k, ids, id_base, oD, oI, scan_ws, st, nullptr, ws.flag)) return rc;
    }
    return WISE_OK;
}

}  // namespace flat_codec
}  // namespace wise

// Sortable 64-bit (score,row) keys shared by the scan kernels and the merge kernels, the id lookup of the reconstruct kernels
// (row_of_id), and what the flat-search files (ip_topk.hip, ip_range.hip, ip_shadow.hip, ip_topk_mfma.hip) share.
#pragma once
#include "common.h"

namespace wise {

typedef unsigned long long u64;

__device__ __forceinline__ unsigned f32_order(float f) {
    unsigned u = __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float f32_unorder(unsigned o) {
    unsigned u = o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu);
    return __uint_as_float(u);
}
// larger key = better: higher score first, then lower row
__device__ __forceinline__ u64 make_key(float score, unsigned row) {
    return ((u64)f32_order(score) << 32) | (u64)(0xFFFFFFFFu - row);
}

// THE ROW OF AN ID (the reconstruct kernels, find_kernel of ivf_pq.hip).  Block-wide: every thread of the block calls it with the
// same arguments and gets the row that carries the id `want`, or -1.  ids == nullptr: the ids are id_base + row.  The highest
// position wins where an id repeats.
__device__ __forceinline__ long long row_of_id(const long long* __restrict__ ids, long long id_base, long long N, long long want) {
    __shared__ unsigned long long s_row1;  // row + 1, 0 = not found
    if (threadIdx.x == 0)
        s_row1 = ids ? 0ull : ((want >= id_base && want - id_base < N) ? (unsigned long long)(want - id_base + 1) : 0ull);
    __syncthreads();
    if (ids) {
        for (long long r = threadIdx.x; r < N; r += blockDim.x)
            if (ids[r] == want) atomicMax(&s_row1, (unsigned long long)(r + 1));
        __syncthreads();
    }
    return (long long)s_row1 - 1;
}

__device__ __forceinline__ void wave_lds_fence() {
    // one wave executes its DS instructions in order; this only stops the compiler reordering them
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Sort buf[0..cap) descending by one wave (cap = power of two >= 64).
__device__ inline void wave_bitonic_desc(volatile u64* buf, int cap, int lane) {
    for (int size = 2; size <= cap; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = lane; t < (cap >> 1); t += 64) {
                int pos = ((t / stride) * (stride << 1)) + (t % stride);
                int par = pos + stride;
                bool desc = ((pos & size) == 0);
                u64 a = buf[pos], b = buf[par];
                bool sw = desc ? (a < b) : (a > b);
                if (sw) { buf[pos] = b; buf[par] = a; }
            }
            wave_lds_fence();
        }
    }
}

// A wave-private running top-k list in LDS.
struct WaveList {
    volatile u64* buf;  // cap entries
    int cap, k, cnt;
    u64 tau;  // keys <= tau cannot enter the top-k any more
    __device__ void init(u64* b, int cap_, int k_, int lane) {
        buf = b; cap = cap_; k = k_; cnt = 0; tau = 0;
        for (int i = lane; i < cap; i += 64) buf[i] = 0;
        wave_lds_fence();
    }
    __device__ void compact(int lane) {
        for (int i = cnt + lane; i < cap; i += 64) buf[i] = 0;
        wave_lds_fence();
        wave_bitonic_desc(buf, cap, lane);
        if (cnt >= k) { cnt = k; tau = buf[k - 1]; }
    }
    // every lane may carry one candidate key (pass=false -> none); wave-uniform control flow
    __device__ void offer(bool pass, u64 key, int lane) {
        u64 mask = __ballot(pass);
        if (mask == 0) return;
        int n = __popcll(mask);
        if (cnt + n > cap) {
            compact(lane);
            // the threshold moved: re-test
            pass = pass && (key > tau);
            mask = __ballot(pass);
            if (mask == 0) return;
            n = __popcll(mask);
        }
        int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
        if (pass) buf[pos] = key;
        cnt += n;
        wave_lds_fence();
    }
};

// THE fp32 SCORE of the VALU scans (ip_scan_kernel, ip_topk.hip, and the range_search kernels, ip_range.hip): lane l of a wave
// holds float4 chunks l, l + 64, ... of a row and of the query; a row's partial is ONE fmaf chain from +0 over the lane's chunks
// in ascending order, then the 64 partials are folded by a butterfly over the lane masks 32, 16, 8, 4, 2, 1.  The R rows of a
// group share the butterfly's first log2 R steps as a transpose (a lane gives away half of its values and sums the other half
// with its partner's), which leaves row reduced_row(lane) in a lane: the adds of a row and their order do not depend on R.
template <int NV, int R>
__device__ __forceinline__ void row_partials(const f32x4 (&x)[R][NV], const float4 (&qv)[NV], float (&a)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float s = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            s = fmaf(x[r][v][0], qv[v].x, s);
            s = fmaf(x[r][v][1], qv[v].y, s);
            s = fmaf(x[r][v][2], qv[v].z, s);
            s = fmaf(x[r][v][3], qv[v].w, s);
        }
        a[r] = s;
    }
}
// which of the R rows a lane holds after rows_reduce
template <int R>
__device__ __forceinline__ int reduced_row(int lane) {
    int myr = 0, bit = 5;
#pragma unroll
    for (int h = R / 2; h >= 1; h >>= 1, --bit) myr += ((lane >> bit) & 1) * h;
    return myr;
}
template <int R>
__device__ __forceinline__ float rows_reduce(float (&a)[R], int lane) {
    constexpr int LOGR = (R == 8) ? 3 : (R == 4) ? 2 : (R == 2) ? 1 : 0;
    // transpose-reduce: after step with mask m, a lane keeps half of its values, each summed
    // with the partner lane's copy
    int bit = 5;
#pragma unroll
    for (int h = R / 2; h >= 1; h >>= 1, --bit) {
        const int m = 1 << bit;
        const bool up = (lane >> bit) & 1;
#pragma unroll
        for (int i = 0; i < h; ++i) {
            float send = up ? a[i] : a[i + h];
            float keep = up ? a[i + h] : a[i];
            a[i] = keep + __shfl_xor(send, m, 64);
        }
    }
    float s = a[0];
#pragma unroll
    for (int m = (32 >> LOGR); m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    return s;
}

// ---- the f32 VALU scan and the merge of its lists (ip_topk.hip)
// topk_list_cap(k) = entries of a WaveList that keeps k keys
int topk_list_cap(int k);
// geometry of one launch of the scan: list entries, queries per pass (1, 2 or 4), blocks, LDS bytes
struct ScanPlan {
    int cap, nq_per_pass, grid;
    size_t lds;
};
ScanPlan plan_scan(long long N, int d, int nq, int k);
// ip_scan_kernel<NV, plan.nq_per_pass> over the N rows of X (pos: over the rows X[pos[i]], i < N) for the plan's queries at Q;
// part [plan.grid][plan.nq_per_pass][k] keys.  gate: the launch does nothing unless *gate != 0.  WISE_E_INVALID where no
// kernel exists for (d, plan.nq_per_pass): the caller words the error.
int launch_f32_scan(const ScanPlan& plan, const float* X, long long N, int d, const float* Q, int k, u64* part, hipStream_t st,
                    const int* gate = nullptr, const long long* pos = nullptr);
// merge_keys_kernel, one block per query: folds the P lists part [P][qstride][k] of queries 0 .. nq - 1 into
// outD/outI [q_off + q][k] (ids == nullptr: id_base + row).  Owns the launch geometry: waves per block, LDS bytes and the
// raise of the LDS limit above 48 KiB.  pcount: optional [nq], the lists that hold keys per query (default: all P).
int launch_merge_keys(const u64* part, int P, int qstride, int nq, int k, const long long* ids, long long id_base, float* outD,
                      long long* outI, int q_off, hipStream_t st, const int* gate = nullptr, const int* pcount = nullptr);
// the last step of the list scans (wise_ivf_scan_f32, wise_ivfpq_scan): part [P][nq][k] keys -> outD/outI [nq][k]
// count: optional [nq], the lists of part that hold keys per query (the rank-local scan); default: all P
int merge_lists_launch(const u64* part, int P, int nq, int k, const long long* ids, float* outD, long long* outI,
                       hipStream_t st, const int* count = nullptr, long long id_base = 0);

// ---- batched (MFMA) scans, ip_topk_mfma.hip
constexpr int MFMA_QB = 32;   // queries per pass (the N of v_mfma_f32_32x32x2_f32)
constexpr int MFMA_KL = 16;   // per-lane list length: the path serves k <= 16
bool mfma_scan_supported(int d, int nq, int k);
int mfma_scan_lists(long long N);                    // P: partial lists per query the scan leaves
size_t mfma_scan_part_bytes(long long N, int k);     // P * MFMA_QB * k keys
constexpr int MFMA_KC = 12;   // largest k the split-bf16 candidate scan serves (16 candidates, exact re-scoring)
bool mfma_split_supported(int d, int nq, int k);
// f32 operands, lists of k <= MFMA_KL entries, scores final (12 < k <= 16)
int mfma_scan_launch(const float* X, long long N, int d, const float* qpad /*[32][d], zero rows past nq*/, int nq,
                     int k, u64* part, hipStream_t st);
// the register-queue split scan over a row range, and the sample-pass threshold (ip_topk_mfma.hip)
int split_scan_launch(const float* X, long long N, long long row_offset, int d, const float* qpad, int nq, u64* part,
                      const u64* tau0, hipStream_t st);
// 64 queries per pass, one list per (block, query): part [split64_lists(N)][64][MFMA_KL]
constexpr int MFMA_QB2 = 64;
int split64_lists(long long N);
bool split64_supported(int d);
int split64_scan_launch(const float* X, long long N, long long row_offset, int d, const float* qpad, int nq, u64* part,
                        const u64* tau0, hipStream_t st, const int* gate = nullptr);
// the pass over the bf16 shadow rows, 128 or 64 queries at a time (d up to 512 / 1024): dump != null -> the scores of the
// (sampled) rows go to dump [qb][N]; otherwise every (query, row) reaching thr[query] is appended to cand [qb][cap],
// counts in ctl [qb][4].  chunk_shift >= 0: N counts SAMPLED rows, evenly spaced chunks of 2^chunk_shift groups of 32 rows,
// chunk_stride groups apart.  The query enters as ONE bf16 piece: its rounding is part of the error bound (query_eps).
bool shadow64_supported(int d);
int shadow_pass_queries(int d);   // queries one pass of the shadow scan carries at this d (0: not served)
int shadow64_scan_launch(const bf16_t* Xb, long long N, int d, const float* qpad, int nq, const float* thr, int* ctl,
                         u64* cand, int cap, hipStream_t st, float* dump = nullptr, int qb = 64, int chunk_shift = -1,
                         long long chunk_stride = 0, long long row_base = 0 /*Xb points at this row of the index*/);
int sample_threshold_launch(const float* cand_scores, const long long* cand_rows, u64* tau0, hipStream_t st,
                            int kl = MFMA_KL, const int* gate = nullptr);
// exact f32 scores of cand_rows [nq][MFMA_KL], ordered, first k -> outD/outI [nq][k]
int rescore_launch(const float* X, int d, const float* Q, const long long* cand_rows, int nq, int k, const long long* ids,
                   long long id_base, float* outD, long long* outI, hipStream_t st, const int* gate = nullptr);

// ---- split-bf16 candidates + exact re-scoring for one pass of nq <= qb queries (qb = 32, or 64 where split64_supported(d)),
// k <= MFMA_KC (ip_topk.hip): sample pass over the first sample_rows rows, merge, threshold, main pass over the other rows,
// merge, re-score.  mq [qb][d]: the staged queries, zero rows past nq.  gate (qb = 64 only): every launch returns at once
// while *gate == 0.
// Rows of the sample pass: its MFMA_KL-th candidate of a query is a threshold nothing in the final top MFMA_KL can fall
// below, so the main pass hardly ever touches its lists.  The two callers keep their own rule for sample_rows (0 = no
// sample pass): wise_ip_topk_f32 takes SPLIT_SAMPLE_ROWS once N >= 8 x that, the gated fallback of the batched shadow
// search twice as many once N >= 16 x SPLIT_SAMPLE_ROWS.
constexpr long long SPLIT_SAMPLE_ROWS = 32768;
struct SplitSlots {          // workspace of a pass
    u64* mpart;              // lists of the sample pass, then of the main pass
    long long* cand_rows;    // [qb][MFMA_KL]
    float* cand_scores;      // [qb][MFMA_KL]
    u64* tau0;               // [64]
};
int split_candidates_pass(const float* X, long long N, int d, const float* mq, int nq, int qb, int k, const long long* ids,
                          long long id_base, float* outD, long long* outI, const SplitSlots& ws, long long sample_rows,
                          hipStream_t st, const int* gate = nullptr);

}  // namespace wise

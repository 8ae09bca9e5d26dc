// Sortable 64-bit (score,row) keys shared by the scan kernels and the merge kernels.
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
    __device__ void offer(bool pass, u64 key, int lane, int max_new) {
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
        (void)max_new;
    }
};

// fold part [P][nq][k] keys (per-block lists of a list scan) into outD/outI [nq][k], ids looked up at the end
// (merge_keys_kernel, ip_topk.hip); topk_list_cap(k) = entries of a WaveList that keeps k keys
int topk_list_cap(int k);
// count: optional [nq], the lists of part that hold keys per query (the rank-local scan); default: all P
// id_base: with ids == nullptr the output is id_base + row
int merge_lists_launch(const u64* part, int P, int nq, int k, const long long* ids, float* outD, long long* outI,
                       hipStream_t st, const int* count = nullptr, long long id_base = 0);

// batched (MFMA) scan, ip_topk_mfma.hip
constexpr int MFMA_QB = 32;   // queries per pass (the N of v_mfma_f32_32x32x2_f32)
constexpr int MFMA_KL = 16;   // per-lane list length: the path serves k <= 16
bool mfma_scan_supported(int d, int nq, int k);
int mfma_scan_lists(long long N);                    // P: partial lists per query the scan leaves
size_t mfma_scan_part_bytes(long long N, int k);     // P * MFMA_QB * k keys
constexpr int MFMA_KC = 12;   // largest k the split-bf16 candidate scan serves (16 candidates, exact re-scoring)
bool mfma_split_supported(int d, int nq, int k);
int mfma_scan_launch(const float* X, long long N, int d, const float* qpad /*[32][d], zero rows past nq*/, int nq,
                     int k, u64* part, bool split, hipStream_t st);
// the register-queue split scan over a row range, and the sample-pass threshold (ip_topk_mfma.hip)
int split_scan_launch(const float* X, long long N, long long row_offset, int d, const float* qpad, int nq, u64* part,
                      const u64* tau0, hipStream_t st);
bool split_direct_enabled();
// 64 queries per pass, one list per (block, query): part [split64_lists(N)][64][MFMA_KL]
constexpr int MFMA_QB2 = 64;
int split64_lists(long long N);
bool split64_supported(int d);
int split64_scan_launch(const float* X, long long N, long long row_offset, int d, const float* qpad, int nq, u64* part,
                        const u64* tau0, hipStream_t st, const int* gate = nullptr);
// the pass over the bf16 shadow rows, 64 or 32 queries at a time (d up to 512 / 1024): dump != null -> the scores of the
// (sampled) rows go to dump [qb][N]; otherwise every (query, row) reaching thr[query] is appended to cand [qb][cap],
// counts in ctl [qb][4].  chunk_shift >= 0: N counts SAMPLED rows, evenly spaced chunks of 2^chunk_shift groups of 32 rows,
// chunk_stride groups apart
bool shadow64_supported(int d);
bool shadow32_supported(int d);
int shadow_pass_queries(int d);   // queries one pass of the shadow scan carries at this d (0: not served)
bool shadow_one_piece();   // the batched scan takes the query as one bf16 piece (its rounding enters the error bound)
int shadow64_scan_launch(const bf16_t* Xb, long long N, int d, const float* qpad, int nq, const float* thr, int* ctl,
                         u64* cand, int cap, hipStream_t st, float* dump = nullptr, int qb = 64, int chunk_shift = -1,
                         long long chunk_stride = 0, long long row_base = 0 /*Xb points at this row of the index*/);
int sample_threshold_launch(const float* cand_scores, const long long* cand_rows, u64* tau0, hipStream_t st,
                            int kl = MFMA_KL, const int* gate = nullptr);
// exact f32 scores of cand_rows [nq][MFMA_KL], ordered, first k -> outD/outI [nq][k]
int rescore_launch(const float* X, int d, const float* Q, const long long* cand_rows, int nq, int k, const long long* ids,
                   long long id_base, float* outD, long long* outI, hipStream_t st, const int* gate = nullptr);

}  // namespace wise

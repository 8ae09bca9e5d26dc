// HP-2: brute-force inner-product scan + top-k for gfx950 (MI355X).
//
// Replaces faiss IndexIDMap{IndexFlatIP}::search as called from the reference at
// src/index/feature_search_index.py:113 and api/routes.py:1407 (semantics: SURVEY.md App. A.3).
//
// Roofline: HBM-bound.  Algorithmic bytes per query batch = N*d*4 (every fp32 row read once).
//
// Kernel 1 (ip_scan_kernel): every wave streams groups of R rows (16 B per lane per load, rows are
//   contiguous so a group is one R*d*4-byte burst), keeps the query chunk(s) it needs in VGPRs, and
//   reduces the R*NQ partial dot products with a butterfly *transpose*-reduce (log-many cross-lane
//   moves for all R rows together, not 6 per row).  Selection is fused: each (score,row) becomes a
//   sortable 64-bit key; a wave appends the keys that beat its running threshold to a wave-private
//   LDS list and re-thresholds (bitonic sort in LDS, wave-synchronous, no block barrier) when the
//   list fills.  Nothing but the k best keys per block ever goes back to HBM.
// Kernel 2 (merge_keys_kernel): one block per query folds the per-block lists into the final
//   top-k with the same threshold lists, then translates row -> external id (IndexIDMap).
// This file: that scan with its inverted-list form, the batched entry (wise_ip_topk_f32: the matrix-core scans of
// ip_topk_mfma.hip for 8 or more queries), dense scores, selection, merges.  range_search: ip_range.hip; the two-stage
// search over a bf16 / int8 shadow: ip_shadow.hip; what they share: topk_common.h.
#include "topk_common.h"

namespace wise {

// ------------------------------------------------------------------------------------------------
// scan kernel: NV = float4 chunks per lane per row (ceil(d/256)), NQ queries, R rows per group
// ------------------------------------------------------------------------------------------------
// SEG = true is the inverted-list form (IndexIVFFlat, wise_ivf_scan_f32): block b serves query b / nprobe and
// scans only the rows of the list named by probes[b] (X holds the lists back to back, list_off their bounds);
// its k keys go to part[(b % nprobe) * nq + b / nprobe] so that merge_keys_kernel folds a query's nprobe lists.
// With `count` (wise_ivf_scan_local_f32) only the first count[q] probes of query q are live: the grid is then taken
// probe-major (block b: probe b / nq of query b % nq), a block past its query's count returns before it touches LDS or
// part, and the merge folds count[q] lists.
// SEL = true restricts either form to a set of rows (IDSelector: csrc/ivf_select.hip builds both descriptions of the set).
// The flat form (wise_ip_topk_pos_f32) scans the rows X[pos[i]], i < N, instead of X[i]: pos is ascending and a key carries
// pos[i], so ties, the merge and the id translation are the unfiltered scan's.  The inverted-list form
// (wise_ivf_scan_sel_f32) tests bit `row` of keep before a row is offered, and a wave whose R rows are all clear skips
// their loads (a ballot: the branch is wave-uniform).  With SEL = false neither field is read.
struct SegArgs {
    const long long* probes;    // [nq][nprobe] list numbers, < 0 = nothing to scan
    const long long* list_off;  // [nlist + 1]
    int nprobe, nq;
    const int* gate;            // optional: the launch does nothing unless *gate != 0 (two-stage search fallback)
    const int* count;           // optional [nq]: live probes per query (the rest of the row is not read)
    const unsigned* keep;       // SEL, inverted-list form: bit (row & 31) of keep[row >> 5] set = the row competes
    const long long* pos;       // SEL, flat form: [N] ascending rows of X to scan
};

template <int NV, int NQ, int R, bool SEG = false, bool SEL = false>
__global__ __launch_bounds__(256) void ip_scan_kernel(const f32x4* __restrict__ X, long long N, int d4,
                                                      const float* __restrict__ Q, int k, int cap,
                                                      u64* __restrict__ part /*[grid][NQ][k]*/, SegArgs seg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (seg.gate && *seg.gate == 0) return;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    u64* lds = reinterpret_cast<u64*>(smem);
    // wave w, query q -> lds + (w*NQ + q)*cap
    long long lo = 0;             // first row of the scanned range; N becomes its end
    size_t slot = blockIdx.x;     // where the block's keys go
    if constexpr (SEG) {
        static_assert(NQ == 1, "one query per block in the inverted-list form");
        int qi, pi;
        if (seg.count) {
            // probe-major: the live blocks (pi < count[qi]) are the head of the grid and spread over every XCD, the dead
            // ones its tail; block-uniform exit, no barrier has been reached yet
            pi = blockIdx.x / seg.nq;
            qi = blockIdx.x - pi * seg.nq;
            if (pi >= seg.count[qi]) return;
        } else {
            qi = blockIdx.x / seg.nprobe;
            pi = blockIdx.x - qi * seg.nprobe;
        }
        const long long l = seg.probes[(size_t)qi * seg.nprobe + pi];
        if (l >= 0) { lo = seg.list_off[l]; N = seg.list_off[l + 1]; } else { N = 0; }
        Q += (size_t)qi * d4 * 4;
        slot = (size_t)pi * seg.nq + qi;
    }

    float4 qv[NQ][NV];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            int c = v * 64 + lane;
            qv[q][v] = (c < d4) ? reinterpret_cast<const float4*>(Q)[(long long)q * d4 + c]
                                : make_float4(0.f, 0.f, 0.f, 0.f);
        }

    WaveList wl[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) wl[q].init(lds + (size_t)(wave * NQ + q) * cap, cap, k, lane);

    const long long ngroups = (N - lo + R - 1) / R;
    const long long gw = SEG ? wave : (long long)blockIdx.x * 4 + wave;
    const long long nw = SEG ? 4 : (long long)gridDim.x * 4;

    // which of the R rows this lane ends up holding after the transpose-reduce
    const int myr = reduced_row<R>(lane);
    constexpr int LOGR = (R == 8) ? 3 : (R == 4) ? 2 : (R == 2) ? 1 : 0;
    const bool owner = (lane & ((64 >> LOGR) - 1)) == 0;

    for (long long g = gw; g < ngroups; g += nw) {
        const long long row0 = lo + g * R;
        bool chosen = true;
        if constexpr (SEL && SEG) {
            const long long r = row0 + myr;
            chosen = r < N && ((seg.keep[r >> 5] >> (r & 31)) & 1u) != 0;
            if (__ballot(chosen) == 0) continue;   // none of the R rows is selected: nothing to load (wave-uniform)
        }
        f32x4 x[R][NV];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            long long row = row0 + r;
            if (row >= N) row = N - 1;  // stay in bounds; masked below
            if constexpr (SEL && !SEG) row = seg.pos[row];   // the selected row: still one contiguous 4 d-byte burst
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                int c = v * 64 + lane;
                if (NV * 64 == d4 || c < d4)
                    x[r][v] = __builtin_nontemporal_load(&X[row * d4 + c]);
                else
                    x[r][v] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            float a[R];
            row_partials<NV, R>(x, qv[q], a);
            const float s = rows_reduce<R>(a, lane);

            const long long row = row0 + myr;
            long long krow = row;                  // what the key carries: the row's true position in X
            if constexpr (SEL && !SEG) krow = seg.pos[row < N ? row : N - 1];
            const u64 key = make_key(s, (unsigned)krow);
            const bool pass = owner && (row < N) && (key > wl[q].tau) && chosen;
            wl[q].offer(pass, key, lane);
        }
    }

    // fold the block's 4 wave lists into wave 0's list, then publish k keys per query
#pragma unroll
    for (int q = 0; q < NQ; ++q) wl[q].compact(lane);
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            for (int w = 1; w < 4; ++w) {
                const u64* other = lds + (size_t)(w * NQ + q) * cap;
                for (int i0 = 0; i0 < k; i0 += 64) {
                    int i = i0 + lane;
                    u64 key = (i < k) ? other[i] : 0;
                    bool pass = (key != 0) && (key > wl[q].tau);
                    wl[q].offer(pass, key, lane);
                }
            }
            wl[q].compact(lane);
            u64* dst = part + (slot * NQ + q) * k;
            for (int i = lane; i < k; i += 64) dst[i] = wl[q].buf[i];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// merge kernel: one block per query, NW waves; part [P][nq_stride][k] keys -> outD/outI [nq][k]
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void merge_keys_kernel(const u64* __restrict__ part, int P, int qstride,
                                                          int k, int cap, const long long* __restrict__ ids,
                                                          long long id_base, float* __restrict__ outD,
                                                          long long* __restrict__ outI, int q_off,
                                                          const int* __restrict__ gate = nullptr, int k_in = 0,
                                                          const int* __restrict__ pcount = nullptr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (gate && *gate == 0) return;
    const int kin = k_in > 0 ? k_in : k;   // keys per input list (the lists may be shorter than the k kept)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nwaves = blockDim.x >> 6;
    const int q = blockIdx.x;
    u64* lds = reinterpret_cast<u64*>(smem);

    WaveList wl;
    wl.init(lds + (size_t)wave * cap, cap, k, lane);
    // the P lists of this query hold P*k keys in all: every offer carries 64 of them (one per lane), whatever k
    // is; waves take 64-key chunks round-robin.  pcount: query q folds only its first pcount[q] lists
    const long long total = (long long)(pcount ? pcount[q] : P) * kin;
    for (long long c0 = (long long)wave * 64; c0 < total; c0 += (long long)nwaves * 64) {
        const long long i = c0 + lane;
        u64 key = 0;
        if (i < total) {
            const int p = (int)(i / kin), j = (int)(i - (long long)p * kin);
            key = part[((size_t)p * qstride + q) * kin + j];
        }
        const bool pass = (key != 0) && (key > wl.tau);
        wl.offer(pass, key, lane);
    }
    wl.compact(lane);
    __syncthreads();
    if (wave == 0) {
        for (int w = 1; w < nwaves; ++w) {
            const u64* other = lds + (size_t)w * cap;
            for (int i0 = 0; i0 < k; i0 += 64) {
                int i = i0 + lane;
                u64 key = (i < k) ? other[i] : 0;
                bool pass = (key != 0) && (key > wl.tau);
                wl.offer(pass, key, lane);
            }
        }
        wl.compact(lane);
        for (int i = lane; i < k; i += 64) {
            u64 key = wl.buf[i];
            float dscore = -3.4028234663852886e38f;
            long long id = -1;
            if (key != 0) {
                unsigned row = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
                dscore = f32_unorder((unsigned)(key >> 32));
                id = ids ? ids[row] : (id_base + (long long)row);
            }
            outD[(size_t)(q_off + q) * k + i] = dscore;
            outI[(size_t)(q_off + q) * k + i] = id;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// probe compaction (wise_ivf_scan_local_f32): one wave per query keeps, in probe order, the probes whose list holds
// rows in this rank's slice (list_off clipped to the slice: most lists are empty there) and writes their count
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void compact_probes_kernel(const long long* __restrict__ probes, int nprobe,
                                                            const long long* __restrict__ list_off, int nlist,
                                                            long long* __restrict__ out, int* __restrict__ count) {
    const int lane = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * nprobe;
    int n = 0;
    for (int i0 = 0; i0 < nprobe; i0 += 64) {
        const int i = i0 + lane;
        const long long l = (i < nprobe) ? probes[base + i] : -1;
        const bool keep = l >= 0 && l < nlist && list_off[l + 1] > list_off[l];
        const u64 m = __ballot(keep);
        if (keep) out[base + n + __popcll(m & ((1ull << lane) - 1ull))] = l;
        n += __popcll(m);
    }
    if (lane == 0) count[blockIdx.x] = n;
}

// ------------------------------------------------------------------------------------------------
// merge of (score,id) partial lists (multi-GPU all-gather result): one wave per query
// key = (order(score), ~slot) where slot = part*k + i keeps "lower part first, then list order"
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void merge_pairs_kernel(const float* __restrict__ inD,
                                                         const long long* __restrict__ inI, int parts, int nq,
                                                         int k, int cap, float* __restrict__ outD,
                                                         long long* __restrict__ outI) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const int q = blockIdx.x;
    WaveList wl;
    wl.init(reinterpret_cast<u64*>(smem), cap, k, lane);
    for (int p = 0; p < parts; ++p) {
        const size_t base = ((size_t)p * nq + q) * k;
        for (int i0 = 0; i0 < k; i0 += 64) {
            int i = i0 + lane;
            bool valid = (i < k) && (inI[base + i] >= 0);
            u64 key = valid ? make_key(inD[base + i], (unsigned)(p * k + i)) : 0;
            bool pass = valid && (key > wl.tau);
            wl.offer(pass, key, lane);
        }
    }
    wl.compact(lane);
    for (int i = lane; i < k; i += 64) {
        u64 key = wl.buf[i];
        float dscore = -3.4028234663852886e38f;
        long long id = -1;
        if (key != 0) {
            unsigned slot = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
            int p = slot / k, j = slot % k;
            size_t src = ((size_t)p * nq + q) * k + j;
            dscore = inD[src];
            id = inI[src];
        }
        outD[(size_t)q * k + i] = dscore;
        outI[(size_t)q * k + i] = id;
    }
}

__global__ void reconstruct_kernel(const float* __restrict__ X, long long N, int d,
                                   const long long* __restrict__ ids, long long id_base,
                                   const long long* __restrict__ qids, int n, float* __restrict__ out) {
    const int i = blockIdx.x;
    const long long row = row_of_id(ids, id_base, N, qids[i]);
    for (int c = threadIdx.x; c < d; c += blockDim.x)
        out[(size_t)i * d + c] = (row >= 0) ? X[row * d + c] : __builtin_nanf("");
}

// ------------------------------------------------------------------------------------------------
// select_topk_kernel: indices of the k largest of n scores, one block per row of scores (the coarse stage of
// IndexIVFFlat when nprobe is large: n = nlist is tens of thousands and k up to 2048, where threshold lists
// stop filtering).  Radix select on the sortable 32-bit score, most significant byte first (4 histogram passes
// find the k-th largest value T and how many elements equal to T still belong), then one ordered compaction:
// everything above T, plus the lowest-indexed ties.  Output: the chosen indices in ascending index order.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void select_topk_kernel(const float* __restrict__ scores, int n, int k,
                                                           long long* __restrict__ out /*[rows][k]*/) {
    __shared__ unsigned hist[256];
    __shared__ unsigned s_prefix, s_remaining;
    __shared__ unsigned wave_cnt[2][16];
    __shared__ unsigned base_gt, base_eq;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = scores + (size_t)blockIdx.x * n;
    long long* dst = out + (size_t)blockIdx.x * k;
    const int kk = k < n ? k : n;
    if (tid == 0) { s_prefix = 0; s_remaining = (unsigned)kk; }
    unsigned mask = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const unsigned prefix = s_prefix;
        for (int i = tid; i < n; i += 1024) {
            const unsigned key = f32_order(row[i]);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned rem = s_remaining, cum = 0;
            int b = 255;
            for (; b > 0; --b) {
                if (cum + hist[b] >= rem) break;
                cum += hist[b];
            }
            s_remaining = rem - cum;          // still to take from bucket b
            s_prefix = prefix | ((unsigned)b << shift);
        }
        mask |= 255u << shift;
        __syncthreads();
    }
    const unsigned T = s_prefix;              // the k-th largest key
    const unsigned take_eq = s_remaining;     // how many elements equal to T belong to the result
    if (tid == 0) { base_gt = 0; base_eq = 0; }
    __syncthreads();
    // ordered compaction, 1024 indices at a time: [greater..., then ties] keeps ascending index order within
    // each class; the two classes are interleaved by position so the output is ascending overall
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + tid;
        const unsigned key = i < n ? f32_order(row[i]) : 0u;
        const bool gt = i < n && key > T, eq = i < n && key == T;
        const unsigned long long mg = __ballot(gt), me = __ballot(eq);
        if (lane == 0) { wave_cnt[0][wave] = __popcll(mg); wave_cnt[1][wave] = __popcll(me); }
        __syncthreads();
        unsigned off_g = base_gt, off_e = base_eq, tot_g = 0, tot_e = 0;
        for (int w = 0; w < 16; ++w) {
            if (w < wave) { off_g += wave_cnt[0][w]; off_e += wave_cnt[1][w]; }
            tot_g += wave_cnt[0][w]; tot_e += wave_cnt[1][w];
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        const unsigned rank_g = off_g + __popcll(mg & below), rank_e = off_e + __popcll(me & below);
        // position in the output = (#greater before me) + (#accepted ties before me)
        if (gt) dst[rank_g + min(rank_e, take_eq)] = i;
        else if (eq && rank_e < take_eq) dst[rank_g + rank_e] = i;
        __syncthreads();
        if (tid == 0) { base_gt += tot_g; base_eq += tot_e; }
        __syncthreads();
    }
    for (int j = kk + tid; j < k; j += 1024) dst[j] = -1;   // fewer than k scores: padding
}

static int next_pow2(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}
// a list must be able to take one 64-wide offer on top of k survivors
static int list_cap(int k) { return next_pow2(k + 64); }

// rows per group of the scan: a group is one 4 d 4-byte burst, and four rows share the butterfly's first two steps
constexpr int SCAN_ROWS = 4;

ScanPlan plan_scan(long long N, int d, int nq, int k) {
    ScanPlan p;
    p.cap = list_cap(k);
    const int nv = (d / 4 + 63) / 64;
    // queries per pass: registers (NV*NQ <= 8 keeps the kernel spill-free) and LDS
    // (4 waves * NQ * cap * 8 B <= 64 KiB so two blocks fit a CU)
    int nqp = 1;
    while (nqp * 2 <= nq && nqp * 2 <= 4 && nv * nqp * 2 <= 8 && (size_t)4 * nqp * 2 * p.cap * 8 <= 64 * 1024) nqp <<= 1;
    p.nq_per_pass = nqp;
    p.lds = (size_t)4 * nqp * p.cap * 8;
    int blocks_per_cu = (p.lds > 40 * 1024) ? 2 : 4;
    // 3-KiB rows (d = 768): a grid of 768 blocks instead of 1024 spreads the row stream over the memory channels —
    // 3.57 -> 4.89 TB/s measured on 6.25M x 768 (grids of 512, 1024 and 2048 blocks all sit at 3.6)
    if (nv == 3 && blocks_per_cu == 4) blocks_per_cu = 3;
    p.grid = 256 * blocks_per_cu;
    long long ngroups = (N + SCAN_ROWS - 1) / SCAN_ROWS;
    long long need = (ngroups + 3) / 4;
    if (need < 1) need = 1;
    if (p.grid > need) p.grid = (int)need;
    return p;
}

template <int NV, int NQ>
static void launch_scan(const ScanPlan& p, const float* X, long long N, int d, const float* Q, int k, u64* part,
                        hipStream_t st, const int* gate, const long long* pos) {
    SegArgs sa{};
    sa.gate = gate;
    sa.pos = pos;   // wise_ip_topk_pos_f32: N counts the entries of pos
    auto kern = pos ? ip_scan_kernel<NV, NQ, SCAN_ROWS, false, true> : ip_scan_kernel<NV, NQ, SCAN_ROWS>;
    if (p.lds > 48 * 1024)
        raise_lds_limit(reinterpret_cast<const void*>(kern), (int)p.lds);
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(256), p.lds, st, reinterpret_cast<const f32x4*>(X), N, d / 4, Q, k,
                       p.cap, part, sa);
}

template <int NV>
static void launch_seg_scan(const float* X, int d, const float* Q, int k, int cap, u64* part, const SegArgs& seg,
                            hipStream_t st) {
    auto kern = seg.keep ? ip_scan_kernel<NV, 1, 4, true, true> : ip_scan_kernel<NV, 1, 4, true>;
    const size_t lds = (size_t)4 * cap * 8;
    if (lds > 48 * 1024)
        raise_lds_limit(reinterpret_cast<const void*>(kern), (int)lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)((long long)seg.nq * seg.nprobe)), dim3(256), lds, st,
                       reinterpret_cast<const f32x4*>(X), 0ll, d / 4, Q, k, cap, part, seg);
}

template <int NV>
static int dispatch_nq(const ScanPlan& p, const float* X, long long N, int d, const float* Q, int k, u64* part,
                       hipStream_t st, const int* gate, const long long* pos) {
    switch (p.nq_per_pass) {
        case 1: launch_scan<NV, 1>(p, X, N, d, Q, k, part, st, gate, pos); return WISE_OK;
        case 2:
            if constexpr (NV * 2 <= 8) { launch_scan<NV, 2>(p, X, N, d, Q, k, part, st, gate, pos); return WISE_OK; }
            break;
        case 4:
            if constexpr (NV * 4 <= 8) { launch_scan<NV, 4>(p, X, N, d, Q, k, part, st, gate, pos); return WISE_OK; }
            break;
    }
    return WISE_E_INVALID;
}

int launch_f32_scan(const ScanPlan& p, const float* X, long long N, int d, const float* Q, int k, u64* part, hipStream_t st,
                    const int* gate, const long long* pos) {
    switch ((d / 4 + 63) / 64) {
        case 1: return dispatch_nq<1>(p, X, N, d, Q, k, part, st, gate, pos);
        case 2: return dispatch_nq<2>(p, X, N, d, Q, k, part, st, gate, pos);
        case 3: return dispatch_nq<3>(p, X, N, d, Q, k, part, st, gate, pos);
        case 4: return dispatch_nq<4>(p, X, N, d, Q, k, part, st, gate, pos);
        case 5: return dispatch_nq<5>(p, X, N, d, Q, k, part, st, gate, pos);
        case 6: return dispatch_nq<6>(p, X, N, d, Q, k, part, st, gate, pos);
        case 7: return dispatch_nq<7>(p, X, N, d, Q, k, part, st, gate, pos);
        case 8: return dispatch_nq<8>(p, X, N, d, Q, k, part, st, gate, pos);
    }
    return WISE_E_INVALID;
}

int launch_merge_keys(const u64* part, int P, int qstride, int nq, int k, const long long* ids, long long id_base, float* outD,
                      long long* outI, int q_off, hipStream_t st, const int* gate, const int* pcount) {
    // 8192 keys of LDS: as many waves (1 .. 16) as lists of cap entries fit
    const int cap = list_cap(k);
    int mw = 8192 / cap;
    if (mw < 1) mw = 1;
    if (mw > 16) mw = 16;
    const size_t mlds = (size_t)mw * cap * 8;
    if (mlds > 48 * 1024)
        raise_lds_limit(reinterpret_cast<const void*>(merge_keys_kernel), (int)mlds);
    hipLaunchKernelGGL(merge_keys_kernel, dim3(nq), dim3(mw * 64), mlds, st, part, P, qstride, k, cap, ids, id_base, outD, outI,
                       q_off, gate, 0, pcount);
    WISE_LAUNCH_CHECK(gate ? "merge_keys_kernel (gated)" : "merge_keys_kernel");
    return WISE_OK;
}

// the two scans of split_candidates_pass: the lists of the sample pass, then of the main pass, in ws.mpart; *nlists = their number
static int split_candidate_scans(const float* X, long long N, int d, const float* mq, int nq, int qb, const SplitSlots& ws,
                                 long long ns, hipStream_t st, const int* gate, int* nlists) {
    auto scan = [&](const float* Xp, long long n, long long row_off, u64* dst, const u64* t0) {
        return qb == MFMA_QB2 ? split64_scan_launch(Xp, n, row_off, d, mq, nq, dst, t0, st, gate)
                              : split_scan_launch(Xp, n, row_off, d, mq, nq, dst, t0, st);
    };
    auto lists_of = [&](long long n) { return qb == MFMA_QB2 ? split64_lists(n) : mfma_scan_lists(n); };
    int p1 = 0, rc;
    if (ns > 0) {
        if ((rc = scan(X, ns, 0, ws.mpart, nullptr))) return rc;
        p1 = lists_of(ns);
        if ((rc = launch_merge_keys(ws.mpart, p1, qb, nq, MFMA_KL, nullptr, 0ll, ws.cand_scores, ws.cand_rows, 0, st, gate))) return rc;
        if ((rc = sample_threshold_launch(ws.cand_scores, ws.cand_rows, ws.tau0, st, MFMA_KL, gate))) return rc;
    }
    if ((rc = scan(X + (size_t)ns * d, N - ns, ns, ws.mpart + (size_t)p1 * qb * MFMA_KL, ns > 0 ? ws.tau0 : nullptr))) return rc;
    *nlists = p1 + lists_of(N - ns);
    return WISE_OK;
}

int split_candidates_pass(const float* X, long long N, int d, const float* mq, int nq, int qb, int k, const long long* ids,
                          long long id_base, float* outD, long long* outI, const SplitSlots& ws, long long sample_rows,
                          hipStream_t st, const int* gate) {
    WISE_CHECK_ARG(qb == MFMA_QB2 || (qb == MFMA_QB && !gate), "split scan: a gated pass carries 64 queries, not %d", qb);
    int nlists = 0, rc;
    if (gate) {
        rc = split_candidate_scans(X, N, d, mq, nq, qb, ws, sample_rows, st, gate, &nlists);
    } else {
        ProfScope prof(PROF_SCAN, (double)N * d * 4.0, st);
        rc = split_candidate_scans(X, N, d, mq, nq, qb, ws, sample_rows, st, gate, &nlists);
    }
    if (rc) return rc;
    // best MFMA_KL candidates per query by approximate score (rows, not ids), then their exact scores
    if ((rc = launch_merge_keys(ws.mpart, nlists, qb, nq, MFMA_KL, nullptr, 0ll, ws.cand_scores, ws.cand_rows, 0, st, gate))) return rc;
    return rescore_launch(X, d, mq, ws.cand_rows, nq, k, ids, id_base, outD, outI, st, gate);
}

}  // namespace wise

using namespace wise;

// The single-pass VALU scan and its merge, up to 4 queries per pass: the fp32 path of wise_ip_topk_f32 and, with pos (N
// then counts its entries), all of wise_ip_topk_pos_f32.  workspace: keys [grid][nq_per_pass][k], then a padded query block.
static int valu_topk(const float* X, long long N, int d, const float* Q, int nq, int k, const int64_t* ids, int64_t id_base,
                     float* outD, int64_t* outI, void* workspace, hipStream_t st, const long long* pos = nullptr) {
    ScanPlan p = plan_scan(N, d, nq, k);
    u64* part = reinterpret_cast<u64*>(workspace);
    float* qpad = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(workspace) +
                                           align_up((size_t)p.grid * p.nq_per_pass * k * sizeof(u64), 256));
    for (int q0 = 0; q0 < nq; q0 += p.nq_per_pass) {
        const int nqa = (nq - q0 < p.nq_per_pass) ? nq - q0 : p.nq_per_pass;
        const float* qptr = Q + (size_t)q0 * d;
        if (nqa < p.nq_per_pass) {
            // ragged tail: replicate the last query so the kernel shape stays fixed (results ignored)
            for (int j = 0; j < p.nq_per_pass; ++j) {
                int srcq = q0 + (j < nqa ? j : nqa - 1);
                hipError_t e = hipMemcpyAsync(qpad + (size_t)j * d, Q + (size_t)srcq * d, (size_t)d * sizeof(float),
                                              hipMemcpyDeviceToDevice, st);
                if (e != hipSuccess) { set_error("ip_topk: memcpy: %s", hipGetErrorString(e)); return (int)e; }
            }
            qptr = qpad;
        }
        if (N > 0) {
            ProfScope prof(PROF_SCAN, (double)N * d * 4.0, st);
            if (int rc = launch_f32_scan(p, X, N, d, qptr, k, part, st, nullptr, pos)) {
                set_error("ip_topk: no kernel for d=%d", d);
                return rc;
            }
            WISE_LAUNCH_CHECK("ip_scan_kernel");
        }
        if (int rc = launch_merge_keys(part, N > 0 ? p.grid : 0, p.nq_per_pass, nqa, k, reinterpret_cast<const long long*>(ids),
                                       (long long)id_base, outD, reinterpret_cast<long long*>(outI), q0, st))
            return rc;
    }
    return WISE_OK;
}

extern "C" size_t wise_ip_topk_workspace_bytes(int64_t N, int d, int nq, int k) {
    if (N < 0 || d < 4 || nq < 1 || k < 1 || k > 2048) return 0;
    ScanPlan p = plan_scan(N, d, nq, k);
    // part keys [grid][nq_per_pass][k] + padded query block
    size_t valu = align_up((size_t)p.grid * p.nq_per_pass * k * sizeof(u64), 256) +
                  align_up((size_t)p.nq_per_pass * d * sizeof(float), 256) + 256;
    if (mfma_scan_supported(d, nq, k)) {
        // the split path keeps MFMA_KL keys per list and a candidate block [32][MFMA_KL] of (score, row)
        // (lists of the sample pass and of the main pass, a 32-key threshold block)
        size_t mf = align_up(2 * mfma_scan_part_bytes(N, MFMA_KL), 256) + align_up((size_t)MFMA_QB2 * d * sizeof(float), 256) +
                    align_up((size_t)MFMA_QB2 * MFMA_KL * 12, 256) + 512 + 256;
        if (mf > valu) valu = mf;
    }
    return valu;
}

extern "C" int wise_ip_topk_f32(const float* X, int64_t N, int d, const float* Q, int nq, int k, const int64_t* ids,
                                int64_t id_base, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes,
                                void* stream) {
    WISE_CHECK_ARG(d >= 4 && d <= 2048 && d % 4 == 0, "ip_topk: d=%d must be a multiple of 4 in [4,2048]", d);
    WISE_CHECK_ARG(k >= 1 && k <= 2048, "ip_topk: k=%d out of [1,2048]", k);
    WISE_CHECK_ARG(nq >= 1 && nq <= 1024, "ip_topk: nq=%d out of [1,1024]", nq);
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll, "ip_topk: N=%lld out of range", (long long)N);
    WISE_CHECK_ARG(Q && outD && outI && (X || N == 0), "ip_topk: null pointer");
    WISE_CHECK_ARG(((uintptr_t)X & 15) == 0 && ((uintptr_t)Q & 15) == 0, "ip_topk: X and Q must be 16-byte aligned");
    size_t need = wise_ip_topk_workspace_bytes(N, d, nq, k);
    if (!workspace || workspace_bytes < need) {
        set_error("ip_topk: workspace %zu < %zu bytes", workspace_bytes, need);
        return WISE_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    if (N > 0 && mfma_scan_supported(d, nq, k)) {
        // batched path: 32 or 64 queries share one pass over X on the matrix cores — k <= MFMA_KC as split-bf16 candidates
        // + exact re-scoring, 12 < k <= 16 on the f32 matrix-core scan
        const bool split = mfma_split_supported(d, nq, k);
        unsigned char* wsb = reinterpret_cast<unsigned char*>(workspace);
        SplitSlots ws;
        ws.mpart = reinterpret_cast<u64*>(wsb);
        size_t off = align_up(2 * mfma_scan_part_bytes(N, MFMA_KL), 256);
        float* mq = reinterpret_cast<float*>(wsb + off);
        off += align_up((size_t)MFMA_QB2 * d * sizeof(float), 256);
        ws.cand_rows = reinterpret_cast<long long*>(wsb + off);
        ws.cand_scores = reinterpret_cast<float*>(wsb + off + (size_t)MFMA_QB2 * MFMA_KL * 8);
        off += align_up((size_t)MFMA_QB2 * MFMA_KL * 12, 256);
        ws.tau0 = reinterpret_cast<u64*>(wsb + off);
        const long long ns = N >= 8 * SPLIT_SAMPLE_ROWS ? SPLIT_SAMPLE_ROWS : 0;
        for (int q0 = 0; q0 < nq;) {
            // 64 at a time while more than 32 remain (d <= 512 keeps both bf16 images of 64 queries in LDS)
            const int qb = (split && split64_supported(d) && nq - q0 > MFMA_QB) ? MFMA_QB2 : MFMA_QB;
            const int nqa = (nq - q0 < qb) ? nq - q0 : qb;
            hipError_t e = hipSuccess;
            if (nqa < qb) e = hipMemsetAsync(mq, 0, (size_t)qb * d * sizeof(float), st);
            if (e == hipSuccess)
                e = hipMemcpyAsync(mq, Q + (size_t)q0 * d, (size_t)nqa * d * sizeof(float), hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) { set_error("ip_topk: query staging: %s", hipGetErrorString(e)); return (int)e; }
            int rc;
            if (split) {
                rc = split_candidates_pass(X, N, d, mq, nqa, qb, k, reinterpret_cast<const long long*>(ids), (long long)id_base,
                                           outD + (size_t)q0 * k, reinterpret_cast<long long*>(outI) + (size_t)q0 * k, ws, ns, st);
            } else {
                {
                    ProfScope prof(PROF_SCAN, (double)N * d * 4.0, st);
                    rc = mfma_scan_launch(X, N, d, mq, nqa, k, ws.mpart, st);
                }
                if (!rc)
                    rc = launch_merge_keys(ws.mpart, mfma_scan_lists(N), MFMA_QB, nqa, k, reinterpret_cast<const long long*>(ids),
                                           (long long)id_base, outD, reinterpret_cast<long long*>(outI), q0, st);
            }
            if (rc) return rc;
            q0 += nqa;
        }
        return WISE_OK;
    }
    return valu_topk(X, N, d, Q, nq, k, ids, id_base, outD, outI, workspace, st);
}

// wise_ip_topk_f32's fp32 scan over the rows X[pos[i]] (an IDSelector resolved to positions: csrc/ivf_select.hip)
extern "C" int wise_ip_topk_pos_f32(const float* X, int64_t N, int d, const int64_t* pos, int64_t n_pos, const float* Q, int nq,
                                    int k, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    WISE_CHECK_ARG(d >= 4 && d <= 2048 && d % 4 == 0, "ip_topk_pos: d=%d must be a multiple of 4 in [4,2048]", d);
    WISE_CHECK_ARG(k >= 1 && k <= 2048, "ip_topk_pos: k=%d out of [1,2048]", k);
    WISE_CHECK_ARG(nq >= 1 && nq <= 1024, "ip_topk_pos: nq=%d out of [1,1024]", nq);
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll && n_pos >= 0 && n_pos <= N, "ip_topk_pos: N=%lld n_pos=%lld out of range",
                   (long long)N, (long long)n_pos);
    WISE_CHECK_ARG(Q && outD && outI && ((X && pos) || n_pos == 0), "ip_topk_pos: null pointer");
    WISE_CHECK_ARG(((uintptr_t)X & 15) == 0 && ((uintptr_t)Q & 15) == 0, "ip_topk_pos: X and Q must be 16-byte aligned");
    const size_t need = wise_ip_topk_workspace_bytes(n_pos, d, nq, k);
    if (!workspace || workspace_bytes < need) {
        set_error("ip_topk_pos: workspace %zu < %zu bytes", workspace_bytes, need);
        return WISE_E_WORKSPACE;
    }
    return valu_topk(X, n_pos, d, Q, nq, k, ids, id_base, outD, outI, workspace, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(pos));
}

// the last step of the list scans (wise_ivf_scan_f32, wise_ivfpq_scan): part [P][nq][k] keys -> outD/outI [nq][k]
int wise::topk_list_cap(int k) { return list_cap(k); }
int wise::merge_lists_launch(const u64* part, int P, int nq, int k, const long long* ids, float* outD, long long* outI,
                             hipStream_t st, const int* count, long long id_base) {
    return launch_merge_keys(part, P, nq, nq, k, ids, id_base, outD, outI, 0, st, nullptr, count);
}

// Workspace of the list scans: the keys [nprobe][nq][k]; the rank-local form adds the compacted probes [nq][nprobe] and
// (for a call without probe_count) the counts [nq].
static size_t ivf_part_bytes(int nq, int nprobe, int k) { return align_up((size_t)nq * nprobe * k * sizeof(u64), 256); }
static size_t ivf_local_probe_bytes(int nq, int nprobe) { return align_up((size_t)nq * nprobe * sizeof(long long), 256); }

extern "C" size_t wise_ivf_scan_workspace_bytes(int nq, int nprobe, int k) {
    if (nq < 1 || nprobe < 1 || k < 1 || k > 2048) return 0;
    return ivf_part_bytes(nq, nprobe, k);
}

extern "C" size_t wise_ivf_scan_local_workspace_bytes(int nq, int nprobe, int k) {
    if (nq < 1 || nprobe < 1 || nprobe > 2048 || k < 1 || k > 2048) return 0;
    return ivf_part_bytes(nq, nprobe, k) + ivf_local_probe_bytes(nq, nprobe) + align_up((size_t)nq * sizeof(int), 256);
}

// Both list scans.  local: the rank-local form for a slice of the list-major array (list_off clipped to the slice): the
// probes whose local segment is empty are compacted away on the device first, so the scan blocks past a query's count
// return at once and the merge folds count[q] lists instead of nprobe.
static int ivf_scan_impl(const char* what, const float* X, int64_t N, int d, const int64_t* list_off, int nlist,
                         const int64_t* ids, const float* Q, int nq, const int64_t* probes, int nprobe, int k, float* outD,
                         int64_t* outI, bool local, int32_t* probe_count, void* workspace, size_t workspace_bytes,
                         void* stream, const uint32_t* keep = nullptr) {
    WISE_CHECK_ARG(d >= 4 && d <= 2048 && d % 4 == 0, "%s: d=%d must be a multiple of 4 in [4,2048]", what, d);
    WISE_CHECK_ARG(k >= 1 && k <= 2048, "%s: k=%d out of [1,2048]", what, k);
    WISE_CHECK_ARG(nq >= 1 && nprobe >= 1 && (!local || nprobe <= 2048) && nlist >= 1 && (long long)nq * nprobe < (1ll << 31),
                   "%s: nq=%d nprobe=%d nlist=%d out of range", what, nq, nprobe, nlist);
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll, "%s: N=%lld out of range", what, (long long)N);
    WISE_CHECK_ARG(Q && outD && outI && list_off && probes && (X || N == 0), "%s: null pointer", what);
    WISE_CHECK_ARG(((uintptr_t)X & 15) == 0 && ((uintptr_t)Q & 15) == 0, "%s: X and Q must be 16-byte aligned", what);
    const size_t need = local ? wise_ivf_scan_local_workspace_bytes(nq, nprobe, k) : wise_ivf_scan_workspace_bytes(nq, nprobe, k);
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace %zu < %zu bytes", what, workspace_bytes, need);
        return WISE_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    unsigned char* wsb = reinterpret_cast<unsigned char*>(workspace);
    u64* part = reinterpret_cast<u64*>(wsb);
    SegArgs seg = {reinterpret_cast<const long long*>(probes), reinterpret_cast<const long long*>(list_off), nprobe, nq};
    seg.keep = keep;
    if (local) {
        long long* live = reinterpret_cast<long long*>(wsb + ivf_part_bytes(nq, nprobe, k));
        int* count = probe_count ? probe_count
                                 : reinterpret_cast<int*>(wsb + ivf_part_bytes(nq, nprobe, k) + ivf_local_probe_bytes(nq, nprobe));
        hipLaunchKernelGGL(compact_probes_kernel, dim3(nq), dim3(64), 0, st, seg.probes, nprobe, seg.list_off, nlist, live, count);
        WISE_LAUNCH_CHECK("compact_probes_kernel");
        seg.probes = live;
        seg.count = count;
    }
    const int cap = list_cap(k);
    switch ((d / 4 + 63) / 64) {
        case 1: launch_seg_scan<1>(X, d, Q, k, cap, part, seg, st); break;
        case 2: launch_seg_scan<2>(X, d, Q, k, cap, part, seg, st); break;
        case 3: launch_seg_scan<3>(X, d, Q, k, cap, part, seg, st); break;
        case 4: launch_seg_scan<4>(X, d, Q, k, cap, part, seg, st); break;
        case 5: launch_seg_scan<5>(X, d, Q, k, cap, part, seg, st); break;
        case 6: launch_seg_scan<6>(X, d, Q, k, cap, part, seg, st); break;
        case 7: launch_seg_scan<7>(X, d, Q, k, cap, part, seg, st); break;
        case 8: launch_seg_scan<8>(X, d, Q, k, cap, part, seg, st); break;
        default: set_error("%s: no kernel for d=%d", what, d); return WISE_E_INVALID;
    }
    WISE_LAUNCH_CHECK("ip_scan_kernel<seg>");
    return merge_lists_launch(part, nprobe, nq, k, reinterpret_cast<const long long*>(ids), outD,
                              reinterpret_cast<long long*>(outI), st, seg.count);
}

extern "C" int wise_ivf_scan_f32(const float* X, int64_t N, int d, const int64_t* list_off, int nlist,
                                 const int64_t* ids, const float* Q, int nq, const int64_t* probes, int nprobe, int k,
                                 float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream) {
    return ivf_scan_impl("ivf_scan", X, N, d, list_off, nlist, ids, Q, nq, probes, nprobe, k, outD, outI, false, nullptr,
                         workspace, workspace_bytes, stream);
}

extern "C" int wise_ivf_scan_sel_f32(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                                     const float* Q, int nq, const int64_t* probes, int nprobe, int k, const uint32_t* keep,
                                     float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream) {
    WISE_CHECK_ARG(keep || N == 0, "ivf_scan_sel: null bitmap");
    return ivf_scan_impl("ivf_scan_sel", X, N, d, list_off, nlist, ids, Q, nq, probes, nprobe, k, outD, outI, false, nullptr,
                         workspace, workspace_bytes, stream, keep);
}

extern "C" int wise_ivf_scan_local_f32(const float* X, int64_t N, int d, const int64_t* list_off, int nlist,
                                       const int64_t* ids, const float* Q, int nq, const int64_t* probes, int nprobe, int k,
                                       float* outD, int64_t* outI, int32_t* probe_count, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    return ivf_scan_impl("ivf_scan_local", X, N, d, list_off, nlist, ids, Q, nq, probes, nprobe, k, outD, outI, true,
                         probe_count, workspace, workspace_bytes, stream);
}

// ------------------------------------------------------------------------------------------------
// Dense scores S[nq, N] = Q . X^T in exact f32 on the matrix cores (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain,
// bit-identical to a scalar loop) — the coarse stage of IndexIVFFlat when nprobe is a sizeable part of nlist (the
// reference's nprobe = 1024 of 31,620 cells, config.py:19 / api/routes.py:899-902): a threshold list stops filtering
// there, so all scores are written and select_topk_kernel picks the nprobe best.
// Block = 4 waves = 128 rows of X x 32 queries; a wave owns a 32 x 32 tile (16 accumulator registers).  X and Q tiles
// go through LDS in 64-column chunks (row stride 65 floats: the MFMA operand read — 32 lanes, 32 different rows, one
// column — is conflict-free).  ~2 x 988 x 8 x 256 MFMAs for 31,620 x 512 x 256 queries: tens of microseconds.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ip_scores_f32_kernel(const float* __restrict__ X, long long N, int d,
                                                            const float* __restrict__ Q, int nq,
                                                            float* __restrict__ S /*[nq][N]*/) {
    constexpr int KC = 64, LD = KC + 1;
    __shared__ float xs[128 * LD];
    __shared__ float qs[32 * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n0 = (long long)blockIdx.x * 128;
    const int q0 = blockIdx.y * 32;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int c0 = 0; c0 < d; c0 += KC) {
        // stage: 128 x 64 floats of X (8 float4 per thread) and 32 x 64 of Q (2 per thread); zero past the edges
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int idx = t * 256 + tid, r = idx >> 4, c4 = (idx & 15) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n0 + r < N && c0 + c4 < d) v = *reinterpret_cast<const float4*>(X + (size_t)(n0 + r) * d + c0 + c4);
            float* dst = xs + r * LD + c4;
            dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int idx = t * 256 + tid, r = idx >> 4, c4 = (idx & 15) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q0 + r < nq && c0 + c4 < d) v = *reinterpret_cast<const float4*>(Q + (size_t)(q0 + r) * d + c0 + c4);
            float* dst = qs + r * LD + c4;
            dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
        }
        __syncthreads();
        const float* xa = xs + (wave * 32 + (lane & 31)) * LD + (lane >> 5);
        const float* qb = qs + (lane & 31) * LD + (lane >> 5);
#pragma unroll 8
        for (int kk = 0; kk < KC; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[kk], qb[kk], acc, 0, 0, 0);   // D[row of X][query]
        __syncthreads();
    }
    // acc[reg]: X row (reg&3) + 8*(reg>>2) + 4*(lane>>5) of the wave's 32, query lane&31
    const int q = q0 + (lane & 31);
    if (q < nq) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const long long n = n0 + wave * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
            if (n < N) S[(size_t)q * N + n] = acc[reg];
        }
    }
}

extern "C" int wise_ip_scores_f32(const float* X, int64_t N, int d, const float* Q, int nq, float* scores, void* stream) {
    WISE_CHECK_ARG(X && Q && scores && N >= 1 && nq >= 1 && nq <= 65535 * 32 && d >= 4 && d % 4 == 0,
                   "ip_scores: bad argument (N=%lld d=%d nq=%d)", (long long)N, d, nq);
    WISE_CHECK_ARG(((uintptr_t)X & 15) == 0 && ((uintptr_t)Q & 15) == 0, "ip_scores: X and Q must be 16-byte aligned");
    hipLaunchKernelGGL(ip_scores_f32_kernel, dim3((unsigned)((N + 127) / 128), (unsigned)((nq + 31) / 32)), dim3(256), 0,
                       (hipStream_t)stream, X, (long long)N, d, Q, nq, scores);
    WISE_LAUNCH_CHECK("ip_scores_f32_kernel");
    return WISE_OK;
}

extern "C" int wise_select_topk_f32(const float* scores, int rows, int n, int k, int64_t* out, void* stream) {
    WISE_CHECK_ARG(scores && out && rows >= 1 && n >= 1 && k >= 1, "select_topk: bad argument");
    hipLaunchKernelGGL(select_topk_kernel, dim3(rows), dim3(1024), 0, (hipStream_t)stream, scores, n, k,
                       reinterpret_cast<long long*>(out));
    WISE_LAUNCH_CHECK("select_topk_kernel");
    return WISE_OK;
}

extern "C" int wise_topk_merge(const float* inD, const int64_t* inI, int parts, int nq, int k, float* outD,
                               int64_t* outI, void* stream) {
    WISE_CHECK_ARG(inD && inI && outD && outI, "topk_merge: null pointer");
    WISE_CHECK_ARG(parts >= 1 && nq >= 1 && k >= 1 && k <= 2048 && (long long)parts * k <= 65536,
                   "topk_merge: parts=%d nq=%d k=%d out of range", parts, nq, k);
    const int cap = list_cap(k);
    const size_t lds = (size_t)cap * 8;
    hipLaunchKernelGGL(merge_pairs_kernel, dim3(nq), dim3(64), lds, (hipStream_t)stream, inD,
                       reinterpret_cast<const long long*>(inI), parts, nq, k, cap, outD,
                       reinterpret_cast<long long*>(outI));
    WISE_LAUNCH_CHECK("merge_pairs_kernel");
    return WISE_OK;
}

extern "C" int wise_reconstruct_batch(const float* X, int64_t N, int d, const int64_t* ids, int64_t id_base,
                                      const int64_t* query_ids, int n, float* out, void* stream) {
    WISE_CHECK_ARG(X && query_ids && out && n >= 0 && d >= 1, "reconstruct_batch: bad argument");
    if (n == 0) return WISE_OK;
    hipLaunchKernelGGL(reconstruct_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, X, (long long)N, d,
                       reinterpret_cast<const long long*>(ids), (long long)id_base,
                       reinterpret_cast<const long long*>(query_ids), n, out);
    WISE_LAUNCH_CHECK("reconstruct_kernel");
    return WISE_OK;
}

// ------------------------------------------------------------------------------------------------
// search_grouped: "the k best GROUPS of rows (videos, shots, files), each with its best row", answered inside the scan.
// Every stored row carries a group; a group's REPRESENTATIVE is its candidate row with the best (score, position) key, and the
// answer is the k groups whose representatives are best, in the order of those keys.  Three stages, every index type:
//   1  *_group_scores   (beside the range kernels they resemble: ip_range.hip, flat_codec_scan.h, ivf_sq.hip)
//                       ord [nq][N] uint32 = f32_order(key score) of every candidate (query, row) — the upper half of make_key
//                       (topk_common.h), from the scans' own scoring routines —, 0 = not a candidate, the keys' own empty value
//   2  wise_group_best  best [nq][G] = per group the maximum of (ord << 32) | (0xFFFFFFFF - row) over its rows, 0 = no candidate
//   3  wise_group_topk  the k largest of a query's G keys (WaveList, merge_keys_kernel), then positions -> (D, I, G)
// A maximum over a set does not depend on the order of the fold and the low half of a key carries the tie rule (the lower
// position wins), so whatever the arrival order the same inputs give the same bytes.  No atomic touches global memory; stage 2
// folds into LDS with atomic maxima, whose result does not depend on their order either.
//
// STAGE 2 reads group_rows [N] — the row positions sorted by (group, position) — and every ord value once.  Element j of
// group_rows belongs to group g iff group_off[g] <= j < group_off[g + 1].  A block owns the tile of GROUP_TILE consecutive
// elements number blockIdx.x and with it the groups that BEGIN in the tile: it folds all their rows, those past the tile's end
// too (the tail of the last group), and skips the head of the tile where it belongs to a group begun earlier.  One-row groups
// and groups of thousands of rows take the same path: 256 threads walk the elements, not the groups.  Which group an element of
// the tile belongs to comes from a max-scan over the tile: the owned groups mark their first element with (index + 1).  Where
// the groups are contiguous runs of rows — a flat index holds a video's frames in store order — group_rows[j] == j and the ord
// reads are coalesced; under any other assignment they are 4-byte gathers.
// ------------------------------------------------------------------------------------------------
#include "topk_common.h"

namespace wise {

constexpr int GROUP_TILE = 2048;          // elements of group_rows a block owns: 8 per thread
constexpr int GROUP_EPT = GROUP_TILE / 256;
constexpr long long GROUP_SELECT_KEYS = 4096;   // keys of `best` a block of the select pass takes at least

// first g in [0, G] with off[g] >= v (G where there is none below)
__device__ __forceinline__ long long group_lower_bound(const long long* __restrict__ off, long long G, long long v) {
    long long lo = 0, hi = G;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (off[mid] >= v) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const u64 other = __shfl_xor(v, o, 64);
        v = other > v ? other : v;
    }
    return v;
}

// every lane may carry one key for the LDS slot g (has = false: none); wave-uniform control flow.  Lanes that share ONE slot —
// a long group — fold in registers first and send one atomic.
__device__ __forceinline__ void group_fold(u64* lbest, bool has, int g, u64 key, int lane) {
    const u64 m = __ballot(has);
    if (m == 0) return;
    const int first = __ffsll((long long)m) - 1;
    const int g0 = __shfl(g, first, 64);
    if (__ballot(has && g != g0) == 0) {
        const u64 top = wave_max_u64(has ? key : 0ull);
        if (lane == first) atomicMax(lbest + g0, top);
    } else if (has) {
        atomicMax(lbest + g, key);
    }
}

// the key of row `row` for one query (oq = the query's row of ord); 0 where the row is no candidate or out of range
__device__ __forceinline__ u64 group_key(const unsigned* __restrict__ oq, long long N, unsigned row) {
    const unsigned o = row < N ? oq[row] : 0u;
    return o ? ((u64)o << 32) | (u64)(0xFFFFFFFFu - row) : 0ull;
}

// grid = ceil(N / GROUP_TILE).  best is cleared by the host: a block writes the groups it owns, and a group that begins nowhere
// (an empty one behind the last row) keeps its 0.  Whatever group_off and group_rows hold, no access leaves the arrays' declared sizes.
__global__ __launch_bounds__(256) void group_best_kernel(const unsigned* __restrict__ ord, long long N, int nq,
                                                         const long long* __restrict__ group_off, const unsigned* __restrict__ group_rows,
                                                         long long G, u64* __restrict__ best) {
    __shared__ unsigned seg[GROUP_TILE];
    __shared__ u64 lbest[GROUP_TILE];
    __shared__ unsigned wtop[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long lo = (long long)blockIdx.x * GROUP_TILE;
    const long long hi = lo + GROUP_TILE < N ? lo + GROUP_TILE : N;
    const long long gA = group_lower_bound(group_off, G, lo), gB = group_lower_bound(group_off, G, hi);
    // the groups that begin in the tile, GROUP_TILE at a time (more than one round only where groups are empty)
    for (long long ga = gA; ga < gB; ga += GROUP_TILE) {                            // block-uniform
        const long long gb = ga + GROUP_TILE < gB ? ga + GROUP_TILE : gB;
        const int ng = (int)(gb - ga);
        for (int i = tid; i < GROUP_TILE; i += 256) seg[i] = 0u;
        __syncthreads();
        for (int i = tid; i < ng; i += 256) {
            const long long o = group_off[ga + i];
            if (o >= lo && o < hi) atomicMax(&seg[(int)(o - lo)], (unsigned)(i + 1));   // empty groups share an offset: the last one has the rows
        }
        __syncthreads();
        {   // inclusive max-scan of seg: thread t holds entries 8 t .. 8 t + 7
            unsigned v[GROUP_EPT], run = 0u;
#pragma unroll
            for (int e = 0; e < GROUP_EPT; ++e) {
                const unsigned s = seg[tid * GROUP_EPT + e];
                run = s > run ? s : run;
                v[e] = run;
            }
            unsigned inc = run;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned up = __shfl_up(inc, o, 64);
                if (lane >= o) inc = up > inc ? up : inc;
            }
            if (lane == 63) wtop[wave] = inc;
            __syncthreads();
            unsigned before = __shfl_up(inc, 1, 64);
            if (lane == 0) before = 0u;
            for (int w = 0; w < wave; ++w) before = wtop[w] > before ? wtop[w] : before;
#pragma unroll
            for (int e = 0; e < GROUP_EPT; ++e) seg[tid * GROUP_EPT + e] = v[e] > before ? v[e] : before;
        }
        __syncthreads();
        // the elements of this round's groups: [e0, e1), of which [e0, min(e1, hi)) lie in the tile and [hi, e1) are the last group's tail
        long long e0 = group_off[ga], e1 = group_off[gb];
        if (e0 < lo) e0 = lo;
        if (e1 > N) e1 = N;
        const long long in_end = e1 < hi ? e1 : hi;
        unsigned row[GROUP_EPT];
        int grp[GROUP_EPT];                                                         // LDS slot of the element's group, -1: not this round's
#pragma unroll
        for (int e = 0; e < GROUP_EPT; ++e) {
            const int i = e * 256 + tid;
            const long long j = lo + i;
            const bool mine = j >= e0 && j < in_end;
            row[e] = mine ? group_rows[j] : 0u;
            grp[e] = mine ? (int)seg[i] - 1 : -1;
        }
        const int tail_grp = (int)seg[GROUP_TILE - 1] - 1;                          // read only where the tile is full (e1 > hi)
        for (int q = 0; q < nq; ++q) {
            const unsigned* oq = ord + (size_t)q * (size_t)N;
            for (int i = tid; i < ng; i += 256) lbest[i] = 0ull;
            __syncthreads();
#pragma unroll
            for (int e = 0; e < GROUP_EPT; ++e) {
                const u64 key = grp[e] >= 0 ? group_key(oq, N, row[e]) : 0ull;
                group_fold(lbest, key != 0ull, grp[e], key, lane);
            }
            if (e1 > hi && tail_grp >= 0) {                                         // block-uniform
                u64 top = 0ull;
                for (long long j = hi + tid; j < e1; j += 256) {
                    const u64 key = group_key(oq, N, group_rows[j]);
                    top = key > top ? key : top;
                }
                group_fold(lbest, top != 0ull, tail_grp, top, lane);
            }
            __syncthreads();
            u64* dst = best + (size_t)q * (size_t)G + (size_t)ga;
            for (int i = tid; i < ng; i += 256) dst[i] = lbest[i];
            __syncthreads();
        }
    }
}

// STAGE 3, first half: grid (P, nq); block (b, q) offers its strided share of best[q][0 .. G) to four wave lists, folds them and
// leaves k keys at part[(b * nq + q) * k] for merge_keys_kernel
__global__ __launch_bounds__(256) void group_select_kernel(const u64* __restrict__ best, long long G, int k, int cap, u64* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.y, nq = gridDim.y;
    u64* lds = reinterpret_cast<u64*>(smem);
    const u64* mine = best + (size_t)q * (size_t)G;
    WaveList wl;
    wl.init(lds + (size_t)wave * cap, cap, k, lane);
    for (long long c0 = ((long long)blockIdx.x * 4 + wave) * 64; c0 < G; c0 += (long long)gridDim.x * 256) {   // wave-uniform
        const long long i = c0 + lane;
        const u64 key = i < G ? mine[i] : 0ull;
        wl.offer(key != 0ull && key > wl.tau, key, lane);
    }
    wl.compact(lane);
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < 4; ++w) {
        const u64* other = lds + (size_t)w * cap;
        for (int i0 = 0; i0 < k; i0 += 64) {
            const int i = i0 + lane;
            const u64 key = i < k ? other[i] : 0ull;
            wl.offer(key != 0ull && key > wl.tau, key, lane);
        }
    }
    wl.compact(lane);
    u64* dst = part + ((size_t)blockIdx.x * nq + q) * k;
    for (int i = lane; i < k; i += 64) dst[i] = wl.buf[i];
}

// STAGE 3, second half: the merge left key scores in D and POSITIONS in I (-1: no group fills the slot).  A position becomes the
// representative's external id and its group's key; flip: the key score -dist becomes the distance again (and the padding
// +3.4028235e38), as l2_flip_kernel has it
__global__ __launch_bounds__(256) void group_finish_kernel(float* __restrict__ D, long long* __restrict__ I, long long* __restrict__ Gk,
                                                           long long n, const int* __restrict__ gid, long long N,
                                                           const long long* __restrict__ group_keys, long long G,
                                                           const long long* __restrict__ ids, long long id_base, int flip) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long pos = I[i];
    long long id = -1, key = -1;
    if (pos >= 0 && pos < N) {
        id = ids ? ids[pos] : id_base + pos;
        const int g = gid[pos];
        if (g >= 0 && g < G) key = group_keys[g];
    }
    I[i] = id;
    Gk[i] = key;
    if (flip) D[i] = -D[i];
}

static int group_select_blocks(long long G) {
    long long p = (G + GROUP_SELECT_KEYS - 1) / GROUP_SELECT_KEYS;
    return (int)(p < 1 ? 1 : p > 512 ? 512 : p);
}
// gid [N] is int32: a group index stops at 2^31 - 1
static bool group_count_ok(int64_t N, int64_t G) { return G >= 0 && G <= N && G <= 0x7FFFFFFFll; }
static bool group_shape_ok(int64_t N, int64_t G, int nq) { return N >= 0 && N < 0xFFFFFFFFll && group_count_ok(N, G) && nq >= 1 && nq <= 65535; }
static size_t group_ord_bytes(int64_t N, int nq) { return align_up((size_t)nq * (size_t)N * sizeof(unsigned), 256); }
static size_t group_best_bytes(int64_t G, int nq) { return align_up((size_t)nq * (size_t)G * sizeof(u64), 256); }
static size_t group_part_bytes(int64_t G, int nq, int k) { return align_up((size_t)group_select_blocks(G) * nq * k * sizeof(u64), 256); }

}  // namespace wise

using namespace wise;

extern "C" size_t wise_group_workspace_bytes(int64_t N, int64_t G, int nq, int k) {
    if (!group_shape_ok(N, G, nq) || k < 1 || k > 2048) return 0;
    return group_ord_bytes(N, nq) + group_best_bytes(G, nq) + group_part_bytes(G, nq, k);
}

extern "C" int wise_group_best(const uint32_t* ord, int64_t N, int nq, const int64_t* group_off, const uint32_t* group_rows, int64_t G,
                               uint64_t* best, void* stream) {
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll, "group_best: N=%lld out of range", (long long)N);
    WISE_CHECK_ARG(group_count_ok(N, G), "group_best: G=%lld out of [0, min(N=%lld, 2^31 - 1)]", (long long)G, (long long)N);
    WISE_CHECK_ARG(nq >= 1 && nq <= 65535, "group_best: nq=%d out of [1,65535]", nq);
    WISE_CHECK_ARG(group_off && ((ord && group_rows) || N == 0) && (best || G == 0), "group_best: null pointer");
    if (G == 0) return WISE_OK;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(best, 0, (size_t)nq * (size_t)G * sizeof(uint64_t), st);
    if (e != hipSuccess) { set_error("group_best: memset: %s", hipGetErrorString(e)); return (int)e; }
    const long long tiles = ((long long)N + GROUP_TILE - 1) / GROUP_TILE;
    ProfScope prof(PROF_SCAN, (double)nq * (4.0 * (double)N + 8.0 * (double)G) + 4.0 * (double)N, st);
    hipLaunchKernelGGL(group_best_kernel, dim3((unsigned)tiles), dim3(256), 0, st, ord, (long long)N, nq,
                       reinterpret_cast<const long long*>(group_off), group_rows, (long long)G, reinterpret_cast<u64*>(best));
    WISE_LAUNCH_CHECK("group_best_kernel");
    return WISE_OK;
}

extern "C" int wise_group_topk(const uint64_t* best, int64_t G, int nq, int k, const int32_t* gid, int64_t N, const int64_t* group_keys,
                               const int64_t* ids, int64_t id_base, int flip, float* outD, int64_t* outI, int64_t* outG, void* workspace,
                               size_t workspace_bytes, void* stream) {
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll, "group_topk: N=%lld out of range", (long long)N);
    WISE_CHECK_ARG(group_count_ok(N, G), "group_topk: G=%lld out of [0, min(N=%lld, 2^31 - 1)]", (long long)G, (long long)N);
    WISE_CHECK_ARG(nq >= 1 && nq <= 65535, "group_topk: nq=%d out of [1,65535]", nq);
    WISE_CHECK_ARG(k >= 1 && k <= 2048, "group_topk: k=%d out of [1,2048]", k);
    WISE_CHECK_ARG(outD && outI && outG && ((best && gid && group_keys) || G == 0), "group_topk: null pointer");
    const size_t need = group_part_bytes(G, nq, k);
    WISE_CHECK_ARG(workspace && workspace_bytes >= need, "group_topk: workspace %zu < %zu bytes", workspace_bytes, need);
    WISE_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "group_topk: the workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    u64* part = reinterpret_cast<u64*>(workspace);
    const int P = G > 0 ? group_select_blocks(G) : 0;
    if (P > 0) {
        const int cap = topk_list_cap(k);
        const size_t lds = (size_t)4 * cap * 8;
        if (lds > 48 * 1024) raise_lds_limit(reinterpret_cast<const void*>(group_select_kernel), (int)lds);
        hipLaunchKernelGGL(group_select_kernel, dim3((unsigned)P, (unsigned)nq), dim3(256), lds, st, reinterpret_cast<const u64*>(best),
                           (long long)G, k, cap, part);
        WISE_LAUNCH_CHECK("group_select_kernel");
    }
    if (int rc = launch_merge_keys(part, P, nq, nq, k, nullptr, 0ll, outD, reinterpret_cast<long long*>(outI), 0, st)) return rc;
    const long long n = (long long)nq * k;
    hipLaunchKernelGGL(group_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, outD, reinterpret_cast<long long*>(outI),
                       reinterpret_cast<long long*>(outG), n, gid, (long long)N, reinterpret_cast<const long long*>(group_keys), (long long)G,
                       reinterpret_cast<const long long*>(ids), (long long)id_base, flip);
    WISE_LAUNCH_CHECK("group_finish_kernel");
    return WISE_OK;
}

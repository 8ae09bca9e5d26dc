// HP-2: search restricted to a set of ids (faiss's SearchParameters(sel=IDSelector...)).  A selector is resolved per index
// into a bitmap over row POSITIONS — rows of X for the flat index, rows in list order for the inverted-file indexes — and the
// scans test it before a row may compete (ip_scan_kernel<.., SEL> in ip_topk.hip, pq_scan_kernel<.., SEL> in ivf_pq.hip):
// a filter applied after the top-k cannot reach beyond rank k.
//   wise_sel_bitmap     bit p = "the external id of row p is selected": one lane per row, the id tested against a sorted,
//                       de-duplicated id list (binary search) or a half-open range, optionally inverted (IDSelectorNot); a
//                       wave's 64 answers are one __ballot, written by lane 0 as two ordinary 32-bit stores — no atomics.
//                       Layout: uint32 words, bit (p & 31) of word p >> 5; the bits past N are zero, also when inverted
//   wise_sel_positions  the ascending list of set positions and their number: popcount per block of 8192 rows, an exclusive
//                       scan of the block counts by one workgroup, then every block scatters its positions behind its offset.
//                       No atomics anywhere, so the output is the same run after run.  The flat index scans this list
//                       (wise_ip_topk_pos_f32): a selected row is one contiguous 4 d-byte burst wherever it lies
#include "common.h"

namespace wise {
namespace ivf_select {

typedef unsigned long long u64;
enum : int { MODE_BATCH = 0, MODE_RANGE = 1 };
constexpr int POS_THREADS = 256;          // a thread per bitmap word: a block covers 8192 rows

__global__ __launch_bounds__(256) void sel_bitmap_kernel(const long long* __restrict__ ids, long long id_base, long long N,
                                                         const long long* __restrict__ sorted, long long n_sorted, long long imin,
                                                         long long imax, int mode, int invert, unsigned* __restrict__ bitmap,
                                                         long long nwords) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    bool hit = false;
    if (p < N) {
        const long long id = ids ? ids[p] : id_base + p;
        if (mode == MODE_RANGE) {
            hit = id >= imin && id < imax;
        } else {
            long long lo = 0, len = n_sorted;              // lower bound of id in sorted[0, n_sorted)
            while (len > 0) {
                const long long half = len >> 1;
                if (sorted[lo + half] < id) { lo += half + 1; len -= half + 1; } else { len = half; }
            }
            hit = lo < n_sorted && sorted[lo] == id;
        }
        hit = hit != (invert != 0);
    }
    const u64 m = __ballot(hit);                           // lanes past N vote 0: the tail bits are zero
    if ((threadIdx.x & 63) == 0) {
        const long long w = p >> 5;                        // p is a multiple of 64 here
        if (w < nwords) bitmap[w] = (unsigned)m;
        if (w + 1 < nwords) bitmap[w + 1] = (unsigned)(m >> 32);
    }
}

// sum over the block of v (every thread returns it); red: POS_THREADS / 64 ints of LDS
__device__ __forceinline__ int block_sum(int v, int* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int w = 0; w < POS_THREADS / 64; ++w) t += red[w];
    return t;
}

__global__ __launch_bounds__(POS_THREADS) void pos_count_kernel(const unsigned* __restrict__ bitmap, long long nwords,
                                                                long long* __restrict__ counts) {
    __shared__ int red[POS_THREADS / 64];
    const long long w = (long long)blockIdx.x * POS_THREADS + threadIdx.x;
    const int t = block_sum(w < nwords ? __popc(bitmap[w]) : 0, red);
    if (threadIdx.x == 0) counts[blockIdx.x] = t;
}

// counts[b] -> the number of set bits in the blocks before b (in place); total[0] = all of them.  One workgroup.
__global__ __launch_bounds__(1024) void pos_scan_kernel(long long* __restrict__ counts, long long nb, long long* __restrict__ total) {
    __shared__ long long wsum[16];
    __shared__ long long carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (long long b0 = 0; b0 < nb; b0 += 1024) {
        const long long b = b0 + tid;
        const long long v = b < nb ? counts[b] : 0;
        long long inc = v;                                  // inclusive scan inside the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        long long before = carry_s;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        if (b < nb) counts[b] = before + inc - v;
        __syncthreads();
        if (tid == 1023) carry_s = before + inc;
        __syncthreads();
    }
    if (tid == 0) total[0] = carry_s;
}

__global__ __launch_bounds__(POS_THREADS) void pos_scatter_kernel(const unsigned* __restrict__ bitmap, long long nwords,
                                                                  const long long* __restrict__ offsets, long long* __restrict__ pos,
                                                                  long long capacity) {
    __shared__ int wsum[POS_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long w = (long long)blockIdx.x * POS_THREADS + threadIdx.x;
    unsigned word = w < nwords ? bitmap[w] : 0u;
    const int c = __popc(word);
    int inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    long long at = offsets[blockIdx.x] + (inc - c);
    for (int v = 0; v < wave; ++v) at += wsum[v];
    while (word) {                                          // ascending bits: ascending positions
        const int bit = __ffs((int)word) - 1;
        if (at < capacity) pos[at] = w * 32 + bit;          // count reports what did not fit
        ++at;
        word &= word - 1;
    }
}

static long long pos_blocks(long long N) {
    const long long nwords = (N + 31) / 32;
    return (nwords + POS_THREADS - 1) / POS_THREADS;
}

}  // namespace ivf_select
}  // namespace wise

using namespace wise;
using namespace wise::ivf_select;

extern "C" int wise_sel_bitmap(const int64_t* ids, int64_t id_base, int64_t N, int mode, const int64_t* sel_ids, int64_t n_sel,
                               int64_t imin, int64_t imax, int invert, uint32_t* bitmap, void* stream) {
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll, "sel_bitmap: N=%lld out of range", (long long)N);
    WISE_CHECK_ARG(mode == MODE_BATCH || mode == MODE_RANGE, "sel_bitmap: mode=%d (0: sorted id list, 1: range)", mode);
    WISE_CHECK_ARG(mode != MODE_BATCH || (n_sel >= 0 && (sel_ids || n_sel == 0)), "sel_bitmap: bad id list");
    WISE_CHECK_ARG(bitmap || N == 0, "sel_bitmap: null bitmap");
    if (N == 0) return WISE_OK;
    hipLaunchKernelGGL(sel_bitmap_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(ids), (long long)id_base, (long long)N,
                       reinterpret_cast<const long long*>(sel_ids), (long long)(mode == MODE_BATCH ? n_sel : 0), (long long)imin,
                       (long long)imax, mode, invert, bitmap, (long long)((N + 31) / 32));
    WISE_LAUNCH_CHECK("sel_bitmap_kernel");
    return WISE_OK;
}

extern "C" size_t wise_sel_positions_workspace_bytes(int64_t N) {
    if (N < 0 || N >= 0xFFFFFFFFll) return 0;
    return align_up((size_t)(pos_blocks(N) + 1) * sizeof(long long), 256);
}

extern "C" int wise_sel_positions(const uint32_t* bitmap, int64_t N, int64_t* pos, int64_t capacity, int64_t* count,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll, "sel_positions: N=%lld out of range", (long long)N);
    WISE_CHECK_ARG(count && capacity >= 0 && ((bitmap && (pos || capacity == 0)) || N == 0), "sel_positions: null pointer");
    const size_t need = wise_sel_positions_workspace_bytes(N);
    if (!workspace || workspace_bytes < need) {
        set_error("sel_positions: workspace %zu < %zu bytes", workspace_bytes, need);
        return WISE_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    long long* offsets = reinterpret_cast<long long*>(workspace);
    const long long nwords = (N + 31) / 32, nb = pos_blocks(N);
    if (nb > 0) {
        hipLaunchKernelGGL(pos_count_kernel, dim3((unsigned)nb), dim3(POS_THREADS), 0, st, bitmap, nwords, offsets);
        WISE_LAUNCH_CHECK("pos_count_kernel");
    }
    hipLaunchKernelGGL(pos_scan_kernel, dim3(1), dim3(1024), 0, st, offsets, nb, reinterpret_cast<long long*>(count));
    WISE_LAUNCH_CHECK("pos_scan_kernel");
    if (nb > 0) {
        hipLaunchKernelGGL(pos_scatter_kernel, dim3((unsigned)nb), dim3(POS_THREADS), 0, st, bitmap, nwords, offsets,
                           reinterpret_cast<long long*>(pos), (long long)capacity);
        WISE_LAUNCH_CHECK("pos_scatter_kernel");
    }
    return WISE_OK;
}

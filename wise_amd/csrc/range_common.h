// range_search ("every row that scores above a radius"): what the count / fill pairs of the three families share
// (wise_ip_range_*, wise_ivf_range_* in ip_range.hip, wise_ivfsq_range_* in ivf_sq.hip).  `static`: each file gets its own copy.
//
// A SEGMENT is what one workgroup of the count pass owns: RANGE_ROWS consecutive rows of X for the flat index, one probed list
// for the inverted-file types.  The count pass scores a segment in chunks of RANGE_ROWS rows, sets a bit per hit in an LDS
// word array (an LDS atomic OR: the bit's place is the row's, nothing depends on arrival order) and publishes the chunk as
// RANGE_WORDS plain 32-bit stores plus one hit count per segment.  range_scan_kernel turns a query's segment counts into
// exclusive offsets (and the query's total); the fill pass reads a segment's words back, lists the set bits in ascending
// order and re-scores only those rows.  No atomic touches global memory and no offset depends on timing: same inputs, same bytes.
//
// Workspace of a call over nq queries:   hit words [nq][wstride] uint32, then segment offsets [nq][ns + 1] int64
//   flat:          ns = ceil(N / RANGE_ROWS), wstride = ns * RANGE_WORDS; word w of a query covers rows 32 w .. 32 w + 31
//   inverted-file: ns = nprobe, wstride = (N >> 5) + nlist + 1; the words of list l start at (list_off[l] >> 5) + l and bit i
//                  is row list_off[l] + i, so two lists never share a word wherever their bounds fall
//                  ((lo >> 5) + ceil(len / 32) <= ((lo + len) >> 5) + 1: the ranges of consecutive lists are disjoint)
#pragma once
#include "topk_common.h"

namespace wise {

constexpr int RANGE_ROWS = 2048;                // rows per chunk
constexpr int RANGE_WORDS = RANGE_ROWS / 32;    // its hit words: one per lane of a wave

static inline long long range_flat_segments(long long N) { return (N + RANGE_ROWS - 1) / RANGE_ROWS; }
static inline long long range_ivf_wstride(long long N, int nlist) { return (N >> 5) + nlist + 1; }
static inline size_t range_hit_bytes(long long nq, long long wstride) { return align_up((size_t)nq * wstride * sizeof(unsigned), 256); }
static inline size_t range_workspace_bytes(long long nq, long long wstride, long long ns) {
    return range_hit_bytes(nq, wstride) + align_up((size_t)nq * (ns + 1) * sizeof(long long), 256);
}

__device__ __forceinline__ void range_mark(unsigned* hb, int i) { atomicOr(&hb[i >> 5], 1u << (i & 31)); }

// wave 0 of a block: the first nwords (<= RANGE_WORDS) words of the LDS array go to dst; returns their set bits (every lane)
__device__ __forceinline__ int range_publish(const unsigned* hb, unsigned* __restrict__ dst, int nwords, int lane) {
    const unsigned word = lane < nwords ? hb[lane] : 0u;
    if (lane < nwords) dst[lane] = word;
    int n = __popc(word);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o, 64);
    return n;
}

// wave 0 of a block: lst[0 .. n) = the set bits of words[0 .. nwords) in ascending order (bit i of word w = 32 w + i); returns n
__device__ __forceinline__ int range_list(const unsigned* __restrict__ words, int nwords, unsigned short* lst, int lane) {
    unsigned word = lane < nwords ? words[lane] : 0u;
    const int c = __popc(word);
    int inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    int at = inc - c;
    while (word) {
        const int bit = __ffs((int)word) - 1;
        lst[at++] = (unsigned short)(lane * 32 + bit);
        word &= word - 1;
    }
    return __shfl(inc, 63, 64);
}

// One workgroup per query: seg[q][0 .. ns) hit counts -> the hits in the segments before each (in place), seg[q][ns] and
// counts[q] = the query's total.  The scan of pos_scan_kernel (ivf_select.hip), a query per block.
static __global__ __launch_bounds__(1024) void range_scan_kernel(long long* __restrict__ seg, long long ns, long long* __restrict__ counts) {
    __shared__ long long wsum[16];
    __shared__ long long carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long* mine = seg + (size_t)blockIdx.x * (ns + 1);
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (long long b0 = 0; b0 < ns; b0 += 1024) {
        const long long b = b0 + tid;
        const long long v = b < ns ? mine[b] : 0;
        long long inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        long long before = carry_s;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        if (b < ns) mine[b] = before + inc - v;
        __syncthreads();
        if (tid == 1023) carry_s = before + inc;
        __syncthreads();
    }
    if (tid == 0) { mine[ns] = carry_s; counts[blockIdx.x] = carry_s; }
}

}  // namespace wise

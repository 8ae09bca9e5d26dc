// remove_ids: stable, in-place compaction of the per-row arrays of an index under a bitmap over row POSITIONS (the layout
// wise_sel_bitmap writes: bit (p & 31) of word p >> 5; the bits past N are ignored here, whatever they hold).
//   wise_compact_plan   plan[s] = the number of kept rows before SEGMENT s (2048 rows = 64 bitmap words), s = 0 .. nseg, so
//                       plan[nseg] is the total, which also goes to count[0]: a popcount per segment (one wave each), then an
//                       exclusive scan by one workgroup (the shape of pos_count_kernel / pos_scan_kernel in ivf_select.hip)
//   wise_compact_rank   out[i] = kept rows strictly before pos[i] = plan[pos >> 11] + the popcounts of the words of that segment
//                       below pos: list_off [nlist + 1] becomes the new offsets in one launch
//   wise_compact_rows   the kept rows of a row-major array move to rows 0 .. kept - 1, in order, in place.  The array is worked
//                       through in ascending CHUNKS of R = scratch_bytes / width rows, two launches per chunk [c0, c1):
//                         gather   every kept row p of the chunk goes to slot rank(p) - rank(c0) of the scratch buffer
//                         settle   the scratch's rank(c1) - rank(c0) rows go to rows rank(c0) .. of the array
//                       A row's destination never lies behind its source, and chunk c's destinations end at rank(c1) <= c1, so
//                       no later chunk's source is overwritten; inside the chunk all sources are read (gather) before any
//                       destination is written (settle), stream order between the two launches being the only ordering used.
//                       Two shortcuts, both decided from the plan alone and the same in every workgroup of a launch:
//                         identity  rank(c1) == c1: nothing was removed up to the end of the chunk, both launches return
//                         direct    rank(c1) <= c0: the destination rows all lie below the chunk, so gather writes them in place
//                                   and settle returns (no workgroup reads what another writes: sources >= c0, destinations < c0)
//                       Bytes per kept row: 0 (identity), 2 width (direct: one read, one write), 4 width through the scratch.
//                       Once scratch_bytes worth of rows have been removed every later chunk is direct.
// No atomic anywhere; a row's place is its rank, computed from popcounts.  Nothing is allocated and nothing is read back.
// Loads of the array are non-temporal (every source byte is read once per call and never again); the scratch is written and
// re-read with plain accesses so that it may stay in the caches between the two launches.  Workgroups take row groups in
// plain ascending order: no workgroup re-reads what another one read, so there is no L2 sharing for an XCD remap to protect.
#include "common.h"

namespace wise {
namespace compact {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
constexpr int SEG_WORDS = 64;             // a plan segment: 64 bitmap words = 2048 rows
constexpr int SEG_ROWS = SEG_WORDS * 32;
constexpr int THREADS = 256;
constexpr int GROUP_BYTES = 16384;        // a gather workgroup takes about this many bytes of rows (at least one bitmap word)

// bitmap word w with the bits of rows >= N cleared; 0 past the last word
__device__ __forceinline__ unsigned keep_word(const unsigned* __restrict__ keep, long long w, long long N) {
    const long long nwords = (N + 31) >> 5;
    if (w >= nwords) return 0u;
    unsigned v = keep[w];
    if (w == nwords - 1 && (N & 31)) v &= (1u << (N & 31)) - 1u;
    return v;
}

// kept rows strictly before pos (0 <= pos <= N), computed by ONE WAVE: every lane returns it
__device__ __forceinline__ long long wave_rank(const unsigned* __restrict__ keep, long long N, const long long* __restrict__ plan,
                                               long long pos) {
    const int lane = threadIdx.x & 63;
    const long long seg = pos >> 11, w = (seg << 6) + lane, pw = pos >> 5;
    unsigned v = 0u;
    if (w < pw) v = keep_word(keep, w, N);
    else if (w == pw && (pos & 31)) v = keep_word(keep, w, N) & ((1u << (pos & 31)) - 1u);
    int c = __popc(v);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
    return plan[seg] + c;
}

__global__ __launch_bounds__(THREADS) void plan_count_kernel(const unsigned* __restrict__ keep, long long N, long long nseg,
                                                             long long* __restrict__ plan) {
    const int lane = threadIdx.x & 63;
    const long long seg = (long long)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    if (seg >= nseg) return;                              // whole waves leave together
    int c = __popc(keep_word(keep, (seg << 6) + lane, N));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) plan[seg] = c;
}

// plan[0 .. nseg) -> exclusive sums in place; plan[nseg] = count[0] = the total.  One workgroup.
__global__ __launch_bounds__(1024) void plan_scan_kernel(long long* __restrict__ plan, long long nseg, long long* __restrict__ count) {
    __shared__ long long wsum[16];
    __shared__ long long carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (long long b0 = 0; b0 < nseg; b0 += 1024) {
        const long long b = b0 + tid;
        const long long v = b < nseg ? plan[b] : 0;
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
        if (b < nseg) plan[b] = before + inc - v;
        __syncthreads();
        if (tid == 1023) carry_s = before + inc;
        __syncthreads();
    }
    if (tid == 0) {
        plan[nseg] = carry_s;
        count[0] = carry_s;
    }
}

// a wave per position
__global__ __launch_bounds__(THREADS) void rank_kernel(const unsigned* __restrict__ keep, long long N, const long long* __restrict__ plan,
                                                       const long long* __restrict__ pos, long long n, long long* __restrict__ out) {
    const long long i = (long long)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    if (i >= n) return;
    long long p = pos[i];
    p = p < 0 ? 0 : (p > N ? N : p);                      // the entry point documents 0 <= pos <= N; never read outside the bitmap
    const long long r = wave_rank(keep, N, plan, p);
    if ((threadIdx.x & 63) == 0) out[i] = r;
}

template <typename V>
__device__ __forceinline__ V load_nt(const V* p) { return __builtin_nontemporal_load(p); }

// Gather the kept rows of chunk [c0, c1).  Workgroup b owns `wpb` bitmap words (a power of two <= 64, so inside one segment)
// starting at word ((c0 >> 5) / wpb + b) * wpb; `vpr` = width / sizeof(V) vectors per row.
template <typename V>
__global__ __launch_bounds__(THREADS) void gather_kernel(V* __restrict__ data, long long N, unsigned vpr, const unsigned* __restrict__ keep,
                                                         const long long* __restrict__ plan, V* __restrict__ scratch, long long c0,
                                                         long long c1, int wpb) {
    __shared__ unsigned short list[SEG_ROWS];             // the kept rows of this workgroup, relative to its first row
    __shared__ unsigned words[SEG_WORDS];
    __shared__ int pre[SEG_WORDS + 1];
    __shared__ long long ranks[3];                        // rank(c0), rank(c1), rank(first row of this workgroup)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long w0 = ((c0 >> 5) / wpb + blockIdx.x) * (long long)wpb, row0 = w0 << 5;
    if (wave < 3) {
        const long long r = wave_rank(keep, N, plan, wave == 0 ? c0 : (wave == 1 ? c1 : row0));
        if (lane == 0) ranks[wave] = r;
    } else {
        // the words of this workgroup restricted to the chunk, and their exclusive popcount sums
        unsigned v = 0u;
        if (lane < wpb) {
            v = keep_word(keep, w0 + lane, N);
            const long long first = row0 + ((long long)lane << 5);
            if (first < c0) v = c0 - first >= 32 ? 0u : v & ~((1u << (c0 - first)) - 1u);
            if (first + 32 > c1) v = c1 <= first ? 0u : v & ((1u << (c1 - first)) - 1u);
        }
        const int c = __popc(v);
        int inc = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        words[lane] = v;
        pre[lane] = inc - c;
        if (lane == 63) pre[SEG_WORDS] = inc;
    }
    __syncthreads();
    const long long r0 = ranks[0], r1 = ranks[1];
    if (r1 == c1) return;                                 // identity: every row below c1 is kept and already in place
    const bool direct = r1 <= c0;
    const int kept = pre[SEG_WORDS];
    if (kept == 0) return;
    if (tid < wpb) {
        unsigned v = words[tid];
        int at = pre[tid];
        while (v) {
            list[at++] = (unsigned short)((tid << 5) + __ffs((int)v) - 1);
            v &= v - 1;
        }
    }
    __syncthreads();
    // the rank of this workgroup's first row counts kept rows of [row0, c0) too when the chunk starts inside it; those bits
    // were cleared above, so start from the larger of the two
    const long long dst0 = (row0 < c0 ? r0 : ranks[2]);
    V* __restrict__ out = direct ? data + (size_t)dst0 * vpr : scratch + (size_t)(dst0 - r0) * vpr;
    const V* __restrict__ in = data + (size_t)row0 * vpr;
    if (vpr >= THREADS) {
        for (int r = 0; r < kept; ++r) {
            const V* __restrict__ s = in + (size_t)list[r] * vpr;
            V* __restrict__ o = out + (size_t)r * vpr;
            unsigned c = tid;
            for (; c + 3 * THREADS < vpr; c += 4 * THREADS) {
                const V a0 = load_nt(s + c), a1 = load_nt(s + c + THREADS), a2 = load_nt(s + c + 2 * THREADS),
                        a3 = load_nt(s + c + 3 * THREADS);
                o[c] = a0; o[c + THREADS] = a1; o[c + 2 * THREADS] = a2; o[c + 3 * THREADS] = a3;
            }
            for (; c < vpr; c += THREADS) o[c] = load_nt(s + c);
        }
    } else {
        const unsigned total = (unsigned)kept * vpr;      // <= 2048 * 255
        unsigned g = tid;
        for (; g + 3 * THREADS < total; g += 4 * THREADS) {
            V a[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const unsigned gu = g + u * THREADS, r = gu / vpr, c = gu - r * vpr;
                a[u] = load_nt(in + (size_t)list[r] * vpr + c);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) out[g + u * THREADS] = a[u];
        }
        for (; g < total; g += THREADS) {
            const unsigned r = g / vpr, c = g - r * vpr;
            out[g] = load_nt(in + (size_t)list[r] * vpr + c);
        }
    }
}

// scratch rows [0, rank(c1) - rank(c0)) -> array rows [rank(c0), rank(c1)); grid-stride
template <typename V>
__global__ __launch_bounds__(THREADS) void settle_kernel(V* __restrict__ data, long long N, unsigned vpr, const unsigned* __restrict__ keep,
                                                         const long long* __restrict__ plan, const V* __restrict__ scratch, long long c0,
                                                         long long c1) {
    __shared__ long long ranks[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (wave < 2) {
        const long long r = wave_rank(keep, N, plan, wave == 0 ? c0 : c1);
        if (lane == 0) ranks[wave] = r;
    }
    __syncthreads();
    const long long r0 = ranks[0], r1 = ranks[1];
    if (r1 == c1 || r1 <= c0) return;                     // identity / direct: gather_kernel has done all there is to do
    const size_t total = (size_t)(r1 - r0) * vpr, step = (size_t)gridDim.x * THREADS;
    V* __restrict__ out = data + (size_t)r0 * vpr;
    size_t g = (size_t)blockIdx.x * THREADS + tid;
    for (; g + 3 * step < total; g += 4 * step) {
        const V a0 = scratch[g], a1 = scratch[g + step], a2 = scratch[g + 2 * step], a3 = scratch[g + 3 * step];
        out[g] = a0; out[g + step] = a1; out[g + 2 * step] = a2; out[g + 3 * step] = a3;
    }
    for (; g < total; g += step) out[g] = scratch[g];
}

static long long segments(long long N) { return (N + SEG_ROWS - 1) / SEG_ROWS; }

template <typename V>
static int compact_rows_t(void* data, long long N, long long width, const unsigned* keep, const long long* plan, void* scratch,
                          long long R, hipStream_t st) {
    const unsigned vpr = (unsigned)(width / (long long)sizeof(V));
    int wpb = 1;
    while (wpb < SEG_WORDS && (long long)wpb * 32 * width < GROUP_BYTES) wpb <<= 1;
    for (long long c0 = 0; c0 < N; c0 += R) {
        const long long c1 = c0 + R < N ? c0 + R : N;
        const long long groups = ((c1 - 1) >> 5) / wpb - (c0 >> 5) / wpb + 1;
        hipLaunchKernelGGL(gather_kernel<V>, dim3((unsigned)groups), dim3(THREADS), 0, st, reinterpret_cast<V*>(data), N, vpr, keep, plan,
                           reinterpret_cast<V*>(scratch), c0, c1, wpb);
        WISE_LAUNCH_CHECK("compact gather_kernel");
        const long long vecs = (c1 - c0) * (long long)vpr;
        long long blocks = (vecs + 4 * THREADS - 1) / (4 * THREADS);
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(settle_kernel<V>, dim3((unsigned)blocks), dim3(THREADS), 0, st, reinterpret_cast<V*>(data), N, vpr, keep, plan,
                           reinterpret_cast<const V*>(scratch), c0, c1);
        WISE_LAUNCH_CHECK("compact settle_kernel");
    }
    return WISE_OK;
}

}  // namespace compact
}  // namespace wise

using namespace wise;
using namespace wise::compact;

extern "C" int64_t wise_compact_plan_entries(int64_t N) {
    if (N < 0 || N >= 0xFFFFFFFFll) return 0;
    return segments(N) + 1;
}

extern "C" int wise_compact_plan(const uint32_t* keep, int64_t N, int64_t* plan, int64_t* count, void* stream) {
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll, "compact_plan: N=%lld out of range", (long long)N);
    WISE_CHECK_ARG(plan && count && (keep || N == 0), "compact_plan: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const long long nseg = segments(N);
    if (nseg > 0) {
        hipLaunchKernelGGL(plan_count_kernel, dim3((unsigned)((nseg + THREADS / 64 - 1) / (THREADS / 64))), dim3(THREADS), 0, st, keep,
                           (long long)N, nseg, reinterpret_cast<long long*>(plan));
        WISE_LAUNCH_CHECK("compact plan_count_kernel");
    }
    hipLaunchKernelGGL(plan_scan_kernel, dim3(1), dim3(1024), 0, st, reinterpret_cast<long long*>(plan), nseg,
                       reinterpret_cast<long long*>(count));
    WISE_LAUNCH_CHECK("compact plan_scan_kernel");
    return WISE_OK;
}

extern "C" int wise_compact_rank(const uint32_t* keep, int64_t N, const int64_t* plan, const int64_t* pos, int64_t n, int64_t* out,
                                 void* stream) {
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll, "compact_rank: N=%lld out of range", (long long)N);
    WISE_CHECK_ARG(n >= 0 && n < 0x7FFFFFFFll, "compact_rank: n=%lld out of range", (long long)n);
    WISE_CHECK_ARG(plan && (keep || N == 0) && ((pos && out) || n == 0), "compact_rank: null pointer");
    if (n == 0) return WISE_OK;
    hipLaunchKernelGGL(rank_kernel, dim3((unsigned)((n + THREADS / 64 - 1) / (THREADS / 64))), dim3(THREADS), 0, (hipStream_t)stream, keep,
                       (long long)N, reinterpret_cast<const long long*>(plan), reinterpret_cast<const long long*>(pos), (long long)n,
                       reinterpret_cast<long long*>(out));
    WISE_LAUNCH_CHECK("compact rank_kernel");
    return WISE_OK;
}

extern "C" int wise_compact_rows(void* data, int64_t N, int64_t width_bytes, const uint32_t* keep, const int64_t* plan, void* scratch,
                                 size_t scratch_bytes, void* stream) {
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll, "compact_rows: N=%lld out of range", (long long)N);
    WISE_CHECK_ARG(width_bytes >= 1 && width_bytes <= 65536, "compact_rows: width_bytes=%lld (1 .. 65536)", (long long)width_bytes);
    if (N == 0) return WISE_OK;
    WISE_CHECK_ARG(data && keep && plan && scratch, "compact_rows: null pointer");
    WISE_CHECK_ARG(scratch_bytes >= (size_t)width_bytes, "compact_rows: scratch of %zu bytes holds no row of %lld bytes", scratch_bytes,
                   (long long)width_bytes);
    long long R = (long long)(scratch_bytes / (size_t)width_bytes);
    if (R > N) R = N;
    if (R > SEG_ROWS) R -= R % SEG_ROWS;                   // whole segments: a chunk's first workgroup starts at the chunk
    // the widest access the width and both bases allow: 16 bytes where everything is 16-byte aligned, else the largest power
    // of two that divides all three
    const uintptr_t bits = (uintptr_t)data | (uintptr_t)scratch | (uintptr_t)width_bytes;
    hipStream_t st = (hipStream_t)stream;
    const long long* pl = reinterpret_cast<const long long*>(plan);
    if ((bits & 15) == 0) return compact_rows_t<u32x4>(data, N, width_bytes, keep, pl, scratch, R, st);
    if ((bits & 7) == 0) return compact_rows_t<u32x2>(data, N, width_bytes, keep, pl, scratch, R, st);
    if ((bits & 3) == 0) return compact_rows_t<unsigned>(data, N, width_bytes, keep, pl, scratch, R, st);
    if ((bits & 1) == 0) return compact_rows_t<unsigned short>(data, N, width_bytes, keep, pl, scratch, R, st);
    return compact_rows_t<unsigned char>(data, N, width_bytes, keep, pl, scratch, R, st);
}

// Selectors that speak in GROUPS (videos, shots, files) and trees of selectors.  Everything here writes or combines bitmaps of the
// layout wise_sel_bitmap (ivf_select.hip) defines — uint32 words, bit (p & 31) of word p >> 5, (N + 31) / 32 words all written, the
// bits past N zero, also when inverted — so every consumer of a resolved selector takes the result as it is.
//   wise_sel_bitmap_groups  bit p = "the group key of row p occurs in sel_keys", from the group tables of set_groups (gid [N] int32,
//                           group_keys [G] ascending).  Two launches: the MARK pass gives every group a lane, which looks its key up
//                           in the sorted sel_keys (binary search) — a wave's 64 answers are one __ballot, G bits into the workspace;
//                           the ROW pass gives every row a lane, which reads gid[p] and tests that group's mark bit — again one
//                           ballot per wave.  The device reads 4 N bytes and writes N / 8; the marks (G / 8 bytes) stay in cache.
//   wise_sel_bitmap_idbits  faiss's IDSelectorBitmap: bit p = bit (id & 7) of bits[id >> 3] for the external id of row p
//   wise_sel_combine        a AND b, a OR b, a XOR b, a AND NOT b, NOT a over whole bitmaps, four words a lane where the three
//                           pointers are 16-byte aligned; the last word is masked, so the tail is zero whatever the inputs' tails
// No atomics anywhere: one lane writes each word, the same bits come out on every run.  Nothing allocates or reads back.
#include "common.h"

namespace wise {
namespace sel_tree {

typedef unsigned long long u64;
enum : int { OP_AND = 0, OP_OR = 1, OP_XOR = 2, OP_ANDNOT = 3, OP_NOT = 4 };
constexpr int THREADS = 256;

// lane 0 of every wave stores the wave's ballot as the two words of its 64 positions; `first` is the wave's first position (a
// multiple of 64).  Lanes past the end voted 0, so the tail bits are zero.
__device__ __forceinline__ void store_ballot(u64 m, long long first, unsigned* __restrict__ words, long long nwords) {
    if ((threadIdx.x & 63) == 0) {
        const long long w = first >> 5;
        if (w < nwords) words[w] = (unsigned)m;
        if (w + 1 < nwords) words[w + 1] = (unsigned)(m >> 32);
    }
}

__global__ __launch_bounds__(THREADS) void mark_groups_kernel(const long long* __restrict__ group_keys, long long G,
                                                              const long long* __restrict__ sel, long long n_sel,
                                                              unsigned* __restrict__ marks, long long nwords) {
    const long long g = (long long)blockIdx.x * THREADS + threadIdx.x;
    bool hit = false;
    if (g < G) {
        const long long key = group_keys[g];
        long long lo = 0, len = n_sel;                         // lower bound of key in sel[0, n_sel)
        while (len > 0) {
            const long long half = len >> 1;
            if (sel[lo + half] < key) { lo += half + 1; len -= half + 1; } else { len = half; }
        }
        hit = lo < n_sel && sel[lo] == key;
    }
    store_ballot(__ballot(hit), g - (threadIdx.x & 63), marks, nwords);
}

__global__ __launch_bounds__(THREADS) void rows_of_groups_kernel(const int* __restrict__ gid, long long N, long long G,
                                                                 const unsigned* __restrict__ marks, int invert,
                                                                 unsigned* __restrict__ bitmap, long long nwords) {
    const long long p = (long long)blockIdx.x * THREADS + threadIdx.x;
    bool hit = false;
    if (p < N) {
        const long long g = gid[p];
        if (g >= 0 && g < G) hit = (marks[g >> 5] >> (g & 31)) & 1u;      // G == 0: no marks are read
        hit = hit != (invert != 0);
    }
    store_ballot(__ballot(hit), p - (threadIdx.x & 63), bitmap, nwords);
}

__global__ __launch_bounds__(THREADS) void idbits_kernel(const long long* __restrict__ ids, long long id_base, long long N,
                                                         const unsigned char* __restrict__ bits, long long n_bytes, int invert,
                                                         unsigned* __restrict__ bitmap, long long nwords) {
    const long long p = (long long)blockIdx.x * THREADS + threadIdx.x;
    bool hit = false;
    if (p < N) {
        const long long id = ids ? ids[p] : id_base + p;
        if (id >= 0 && (id >> 3) < n_bytes) hit = (bits[id >> 3] >> (id & 7)) & 1u;
        hit = hit != (invert != 0);
    }
    store_ballot(__ballot(hit), p - (threadIdx.x & 63), bitmap, nwords);
}

__device__ __forceinline__ unsigned combine_word(unsigned a, unsigned b, int op) {
    switch (op) {
        case OP_AND: return a & b;
        case OP_OR: return a | b;
        case OP_XOR: return a ^ b;
        case OP_ANDNOT: return a & ~b;
        default: return ~a;
    }
}

// a lane owns the words [4 t, 4 t + 4): it reads them all before it writes any, so out may be a or b.  VEC: every pointer is
// 16-byte aligned and whole groups of four go as one 16-byte access.  (No __restrict__: the bitmaps may be the same memory.)
template <bool VEC>
__global__ __launch_bounds__(THREADS) void combine_kernel(const unsigned* a, const unsigned* b, unsigned* out, long long nwords,
                                                          unsigned last_mask, int op) {
    const long long w0 = ((long long)blockIdx.x * THREADS + threadIdx.x) * 4;
    if (w0 >= nwords) return;
    const bool two = op != OP_NOT;
    if (VEC && w0 + 4 <= nwords) {
        const uint4 va = *reinterpret_cast<const uint4*>(a + w0);
        const uint4 vb = two ? *reinterpret_cast<const uint4*>(b + w0) : make_uint4(0u, 0u, 0u, 0u);
        uint4 r;
        r.x = combine_word(va.x, vb.x, op);
        r.y = combine_word(va.y, vb.y, op);
        r.z = combine_word(va.z, vb.z, op);
        r.w = combine_word(va.w, vb.w, op);
        if (w0 + 4 == nwords) r.w &= last_mask;
        *reinterpret_cast<uint4*>(out + w0) = r;
        return;
    }
    const int n = (int)(nwords - w0 < 4 ? nwords - w0 : 4);
    unsigned r[4];
    for (int i = 0; i < n; ++i) r[i] = combine_word(a[w0 + i], two ? b[w0 + i] : 0u, op);
    if (w0 + n == nwords) r[n - 1] &= last_mask;
    for (int i = 0; i < n; ++i) out[w0 + i] = r[i];
}

static unsigned grid_of(long long items) { return (unsigned)((items + THREADS - 1) / THREADS); }
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace sel_tree
}  // namespace wise

using namespace wise;
using namespace wise::sel_tree;

extern "C" size_t wise_sel_groups_workspace_bytes(int64_t G) {
    if (G < 0 || G > 0x7FFFFFFFll) return 0;
    const size_t words = (size_t)((G + 31) / 32);
    return align_up((words ? words : 1) * sizeof(uint32_t), 256);
}

extern "C" int wise_sel_bitmap_groups(const int32_t* gid, int64_t N, const int64_t* group_keys, int64_t G, const int64_t* sel_keys,
                                      int64_t n_sel, int invert, uint32_t* bitmap, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll, "sel_bitmap_groups: N=%lld out of range", (long long)N);
    WISE_CHECK_ARG(G >= 0 && G <= 0x7FFFFFFFll, "sel_bitmap_groups: G=%lld out of range (gid is int32)", (long long)G);
    WISE_CHECK_ARG(n_sel >= 0, "sel_bitmap_groups: n_sel=%lld", (long long)n_sel);
    if (N == 0) return WISE_OK;                                // no rows: no words to write
    WISE_CHECK_ARG(gid && bitmap, "sel_bitmap_groups: null gid or bitmap");
    WISE_CHECK_ARG(group_keys || G == 0, "sel_bitmap_groups: null group_keys");
    WISE_CHECK_ARG(sel_keys || n_sel == 0, "sel_bitmap_groups: null sel_keys");
    const size_t need = wise_sel_groups_workspace_bytes(G);
    WISE_CHECK_ARG(workspace && workspace_bytes >= need, "sel_bitmap_groups: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    unsigned* marks = reinterpret_cast<unsigned*>(workspace);
    if (G > 0) {
        hipLaunchKernelGGL(mark_groups_kernel, dim3(grid_of(G)), dim3(THREADS), 0, st, reinterpret_cast<const long long*>(group_keys),
                           (long long)G, reinterpret_cast<const long long*>(sel_keys), (long long)n_sel, marks, (long long)((G + 31) / 32));
        WISE_LAUNCH_CHECK("mark_groups_kernel");
    }
    hipLaunchKernelGGL(rows_of_groups_kernel, dim3(grid_of(N)), dim3(THREADS), 0, st, gid, (long long)N, (long long)G, marks, invert, bitmap,
                       (long long)((N + 31) / 32));
    WISE_LAUNCH_CHECK("rows_of_groups_kernel");
    return WISE_OK;
}

extern "C" int wise_sel_bitmap_idbits(const int64_t* ids, int64_t id_base, int64_t N, const uint8_t* bits, int64_t n_bytes, int invert,
                                      uint32_t* bitmap, void* stream) {
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll, "sel_bitmap_idbits: N=%lld out of range", (long long)N);
    WISE_CHECK_ARG(n_bytes >= 0, "sel_bitmap_idbits: n_bytes=%lld", (long long)n_bytes);
    if (N == 0) return WISE_OK;
    WISE_CHECK_ARG(bitmap, "sel_bitmap_idbits: null bitmap");
    WISE_CHECK_ARG(bits || n_bytes == 0, "sel_bitmap_idbits: null bits");
    hipLaunchKernelGGL(idbits_kernel, dim3(grid_of(N)), dim3(THREADS), 0, (hipStream_t)stream, reinterpret_cast<const long long*>(ids),
                       (long long)id_base, (long long)N, bits, (long long)n_bytes, invert, bitmap, (long long)((N + 31) / 32));
    WISE_LAUNCH_CHECK("idbits_kernel");
    return WISE_OK;
}

extern "C" int wise_sel_combine(const uint32_t* a, const uint32_t* b, int64_t N, int op, uint32_t* out, void* stream) {
    WISE_CHECK_ARG(N >= 0 && N < 0xFFFFFFFFll, "sel_combine: N=%lld out of range", (long long)N);
    WISE_CHECK_ARG(op >= OP_AND && op <= OP_NOT, "sel_combine: op=%d (0: and, 1: or, 2: xor, 3: and-not, 4: not)", op);
    if (N == 0) return WISE_OK;
    WISE_CHECK_ARG(a && out && (b || op == OP_NOT), "sel_combine: null bitmap");
    const long long nwords = (N + 31) / 32;
    const unsigned last_mask = (N & 31) ? ((1u << (N & 31)) - 1u) : 0xFFFFFFFFu;
    const bool vec = aligned16(a) && aligned16(out) && (op == OP_NOT || aligned16(b));
    const dim3 grid(grid_of((nwords + 3) / 4)), block(THREADS);
    if (vec)
        hipLaunchKernelGGL(combine_kernel<true>, grid, block, 0, (hipStream_t)stream, a, b, out, nwords, last_mask, op);
    else
        hipLaunchKernelGGL(combine_kernel<false>, grid, block, 0, (hipStream_t)stream, a, b, out, nwords, last_mask, op);
    WISE_LAUNCH_CHECK("combine_kernel");
    return WISE_OK;
}

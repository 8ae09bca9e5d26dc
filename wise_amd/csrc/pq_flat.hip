// IndexPQ<m>: exhaustive search over 8-bit product-quantizer codes kept in row order (faiss IndexPQ, inner product, no lists).
//   wise_pqflat_topk      THE HOT PATH: score(row) = +0 + sum_j lut[j][code_j], added in that order in fp32 — the bits
//                         wise_ivfpq_scan (ivf_pq.hip) gives a row of a list whose bias is +0 — top-k per query
//   wise_pqflat_topk_pos  the same scan over the rows codes[pos[i]] (a selector's positions)
//   wise_pqflat_decode    reconstruct_batch: concat_j cb[j][code_j]
// The grid runs over row ranges: wave w of block b takes rows (b W + w) 64 .. + 64, then strides by the whole grid (W waves a
// block), so one block's B = 64 W rows are followed by the next block's.  A block first copies the tables of its pass's NQ
// queries (NQ m KiB) into LDS; then one lane scores one row: the row's m bytes are loaded once, in loads of 16, 8, 4 or 1
// bytes — all of a row's loads before its first lookup, and the next row's before this row's lookups — and each of the NQ
// queries runs its own chain of m random ds_read_b32 lookups.  One lane per row is what the fixed
// order of the sum implies.  Selection is the flat scan's: sortable (score, position) keys against per-wave threshold lists,
// folded per block, then merge_keys_kernel (ip_topk.hip).  No atomics, no packed f32 math.
// The table is per block, so the waves that hide the LDS latency must come from the block: plan_pass takes up to 16 waves
// (1024 threads) around one table set and gives waves up before queries only below 4.
#include "topk_common.h"

namespace wise {
namespace pq_flat {

constexpr int KSUB = 256;                 // codewords per sub-space (nbits = 8)
constexpr int LDS_MAX = 160 * 1024;       // one workgroup may take the whole CU's LDS
constexpr int MAX_NQ = 4;                 // queries whose tables share a pass
constexpr int MAX_WAVES = 16;

// A row's m code bytes in registers: VEC bytes a load (m % VEC == 0, rows VEC-aligned because the base is 16-byte aligned), every
// load of the row issued before the first byte is used, so that a lane has its whole row (and, in the scan's loop, the next row)
// in flight at once.  m is wave-uniform: the guards are scalar branches.  VEC = 1 (m not a multiple of 4) reads bytes as it goes.
template <int VEC>
struct RowCodes {
    static constexpr int LOADS = VEC == 1 ? 1 : 128 / VEC;               // m <= 128
    using word_t = unsigned __attribute__((ext_vector_type(VEC == 1 ? 1 : VEC / 4)));
    word_t w[LOADS];
    const unsigned char* row;
    __device__ __forceinline__ void load(const unsigned char* __restrict__ r, int m) {
        row = r;
        if constexpr (VEC > 1) {
#pragma unroll
            for (int u = 0; u < LOADS; ++u)
                if (u * VEC < m) w[u] = __builtin_nontemporal_load(reinterpret_cast<const word_t*>(r + u * VEC));
        }
    }
};

// the NQ scores of one row: per query acc = acc + tab[q][j][code_j], j ascending: the contract's order
template <int VEC, int NQ>
__device__ __forceinline__ void pq_row_scores(const RowCodes<VEC>& c, int m, const float* __restrict__ tab, float (&acc)[NQ]) {
    const int qs = m * KSUB;              // floats between two queries' tables
    if constexpr (VEC == 1) {
        for (int j = 0; j < m; ++j) {
            const unsigned code = c.row[j];
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[q] += tab[q * qs + j * KSUB + code];
        }
    } else {
#pragma unroll
        for (int u = 0; u < RowCodes<VEC>::LOADS; ++u) {
            if (u * VEC < m) {
#pragma unroll
                for (int b = 0; b < VEC; ++b) {
                    const unsigned code = (c.w[u][b >> 2] >> (8 * (b & 3))) & 255u;
#pragma unroll
                    for (int q = 0; q < NQ; ++q) acc[q] += tab[q * qs + (u * VEC + b) * KSUB + code];
                }
            }
        }
    }
}

// grid = blocks over row ranges; part [grid][NQ][k] keys for merge_keys_kernel.  POS: item i is row pos[i] (n counts items; a
// position outside [0, N) is no row at all), and the key carries the row, so ties still go to the lower position
template <int VEC, int NQ, bool POS>
__global__ __launch_bounds__(1024) void pqflat_scan_kernel(const unsigned char* __restrict__ codes, long long N, long long n, int m,
                                                           const long long* __restrict__ pos, const float* __restrict__ lut, int k,
                                                           int cap, u64* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    float* tab = reinterpret_cast<float*>(smem);
    u64* lists = reinterpret_cast<u64*>(smem + (size_t)NQ * m * KSUB * 4);
    const long long stride = (long long)gridDim.x * nwaves * 64;
    long long i0 = ((long long)blockIdx.x * nwaves + wave) * 64;
    // item i of this lane: (its row, whether it is one)
    auto item = [&](long long i, long long& row) {
        bool live = i < n;
        row = i;
        if constexpr (POS) {
            row = live ? pos[i] : 0;
            live = live && row >= 0 && row < N;
        }
        return live;
    };
    long long row;
    bool live = item(i0 + lane, row);
    RowCodes<VEC> cur;
    if (live) cur.load(codes + (size_t)row * m, m);     // the first row's bytes travel while the tables are copied
    {
        const float4* src = reinterpret_cast<const float4*>(lut);
        float4* dst = reinterpret_cast<float4*>(tab);
        for (int i = threadIdx.x; i < NQ * m * (KSUB / 4); i += blockDim.x) dst[i] = src[i];
    }
    WaveList wl[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) wl[q].init(lists + (size_t)(wave * NQ + q) * cap, cap, k, lane);
    __syncthreads();
    for (; i0 < n; i0 += stride) {                                                                     // wave-uniform
        long long row_next;
        const bool live_next = item(i0 + stride + lane, row_next);
        RowCodes<VEC> nxt;
        if (live_next) nxt.load(codes + (size_t)row_next * m, m);                                     // in flight during the lookups
        float s[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) s[q] = 0.f;
        if (live) pq_row_scores<VEC, NQ>(cur, m, tab, s);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const u64 key = make_key(s[q], (unsigned)row);
            wl[q].offer(live && key > wl[q].tau, key, lane);
        }
        cur = nxt;
        row = row_next;
        live = live_next;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) wl[q].compact(lane);
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            for (int w = 1; w < nwaves; ++w) {
                const u64* other = lists + (size_t)(w * NQ + q) * cap;
                for (int i0 = 0; i0 < k; i0 += 64) {
                    const int i = i0 + lane;
                    const u64 key = i < k ? other[i] : 0;
                    wl[q].offer(key != 0 && key > wl[q].tau, key, lane);
                }
            }
            wl[q].compact(lane);
            u64* dst = part + ((size_t)blockIdx.x * NQ + q) * k;
            for (int i = lane; i < k; i += 64) dst[i] = wl[q].buf[i];
        }
    }
}

// out[i][:] = concat_j cb[j][codes[pos[i]][j]]; NaN when pos[i] is out of range
__global__ __launch_bounds__(256) void pqflat_decode_kernel(const unsigned char* __restrict__ codes, long long N,
                                                            const long long* __restrict__ pos, const float* __restrict__ cbs, int d,
                                                            int m, float* __restrict__ out) {
    const int dsub = d / m;
    const long long p = pos[blockIdx.x];
    float* o = out + (size_t)blockIdx.x * d;
    if (p < 0 || p >= N) {
        for (int c = threadIdx.x; c < d; c += blockDim.x) o[c] = __builtin_nanf("");
        return;
    }
    const unsigned char* code = codes + (size_t)p * m;
    for (int c = threadIdx.x; c < d; c += blockDim.x) {
        const int j = c / dsub, t = c - j * dsub;
        o[c] = cbs[((size_t)j * KSUB + code[j]) * dsub + t];
    }
}

struct PassPlan {
    int nq, waves, cap, grid;
    size_t lds;
};
// The geometry of a pass of up to nq_left queries over n items.  Queries: the largest of {4, 2, 1} (not above nq_left) whose
// tables (NQ m KiB) leave room for the lists of at least 4 waves; where not even one query does, one query with the waves that
// fit.  Waves: the most of {16, 8, 4, 2, 1} that fit beside the tables.  Blocks: as many as are resident at once (LDS and
// 2048 threads a CU), or fewer where the rows run out.
static bool plan_pass(long long n, int m, int nq_left, int k, PassPlan* p) {
    if (m < 1 || m > 128 || k < 1 || k > 2048 || nq_left < 1) return false;
    p->cap = topk_list_cap(k);
    const size_t list = (size_t)p->cap * 8;
    auto fits = [&](int nq, int w) { return (size_t)nq * m * KSUB * 4 + (size_t)w * nq * list <= (size_t)LDS_MAX; };
    int nq = MAX_NQ;
    while (nq > nq_left) nq >>= 1;
    while (nq > 1 && !fits(nq, 4)) nq >>= 1;
    int w = MAX_WAVES;
    while (w > 1 && !fits(nq, w)) w >>= 1;
    if (!fits(nq, w)) return false;
    p->nq = nq;
    p->waves = w;
    p->lds = (size_t)nq * m * KSUB * 4 + (size_t)w * nq * list;
    int per_cu = (int)((size_t)LDS_MAX / p->lds);
    if (per_cu > 2048 / (w * 64)) per_cu = 2048 / (w * 64);
    if (per_cu < 1) per_cu = 1;
    if (per_cu > 4) per_cu = 4;
    p->grid = 256 * per_cu;
    long long need = (n + (long long)w * 64 - 1) / ((long long)w * 64);
    if (need < 1) need = 1;
    if (p->grid > need) p->grid = (int)need;
    return true;
}

// the passes a search of nq queries makes: the first takes plan_pass(nq), the later ones what is left
static size_t part_bytes(long long n, int m, int nq, int k) {
    size_t keys = 0;
    for (int left = nq; left > 0;) {
        PassPlan p;
        if (!plan_pass(n, m, left, k, &p)) return 0;
        const size_t v = (size_t)p.grid * p.nq * k;
        if (v > keys) keys = v;
        if (p.nq == 1) break;             // every later pass has this geometry
        left -= (left / p.nq) * p.nq;     // the passes of this geometry
    }
    return align_up(keys * sizeof(u64), 256) + 256;
}

template <int VEC, int NQ>
static void launch_scan(const PassPlan& p, const unsigned char* codes, long long N, long long n, int m, const long long* pos,
                        const float* lut, int k, u64* part, hipStream_t st) {
    auto kern = pos ? pqflat_scan_kernel<VEC, NQ, true> : pqflat_scan_kernel<VEC, NQ, false>;
    if (p.lds > 48 * 1024) raise_lds_limit(reinterpret_cast<const void*>(kern), (int)p.lds);
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(p.waves * 64), p.lds, st, codes, N, n, m, pos, lut, k, p.cap, part);
}

template <int VEC>
static void dispatch_nq(const PassPlan& p, const unsigned char* codes, long long N, long long n, int m, const long long* pos,
                        const float* lut, int k, u64* part, hipStream_t st) {
    if (p.nq == 4) launch_scan<VEC, 4>(p, codes, N, n, m, pos, lut, k, part, st);
    else if (p.nq == 2) launch_scan<VEC, 2>(p, codes, N, n, m, pos, lut, k, part, st);
    else launch_scan<VEC, 1>(p, codes, N, n, m, pos, lut, k, part, st);
}

static bool shape_ok(int64_t N, int m, int nq, int k) {
    return N >= 0 && N < 0xFFFFFFFFll && m >= 1 && m <= 128 && nq >= 0 && k >= 1 && k <= 2048;
}

// wise_pqflat_topk (pos == nullptr: the rows 0 .. N - 1) and wise_pqflat_topk_pos (the n rows pos[])
static int topk_impl(const char* what, const uint8_t* codes, int64_t N, int m, const int64_t* pos, int64_t n, bool by_pos, const float* lut,
                     int nq, int k, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI, void* workspace,
                     size_t workspace_bytes, void* stream) {
    if (!shape_ok(N, m, nq, k)) {
        set_error("%s: N=%lld m=%d nq=%d k=%d unsupported (N < 2^32 - 1, 1 <= m <= 128, nq >= 0, 1 <= k <= 2048)", what, (long long)N, m, nq, k);
        return WISE_E_UNSUPPORTED;
    }
    WISE_CHECK_ARG(!by_pos || (n >= 0 && n <= N && (pos || n == 0)), "%s: n_pos=%lld out of [0, N] or null pos", what, (long long)n);
    if (nq == 0) return WISE_OK;
    WISE_CHECK_ARG(lut && outD && outI && (codes || N == 0), "%s: null pointer", what);
    WISE_CHECK_ARG(((uintptr_t)codes & 15) == 0 && ((uintptr_t)lut & 15) == 0, "%s: codes and lut must be 16-byte aligned", what);
    const size_t need = part_bytes(n, m, nq, k);
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace %zu < %zu bytes", what, workspace_bytes, need);
        return WISE_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    u64* part = reinterpret_cast<u64*>(workspace);
    const long long* pp = by_pos ? reinterpret_cast<const long long*>(pos) : nullptr;
    for (int q0 = 0; q0 < nq;) {
        PassPlan p;
        if (!plan_pass(n, m, nq - q0, k, &p)) return WISE_E_UNSUPPORTED;
        const float* lp = lut + (size_t)q0 * m * KSUB;
        if (n > 0) {
            ProfScope prof(PROF_SCAN, (double)n * (double)m, st);
            if (m % 16 == 0) dispatch_nq<16>(p, codes, N, n, m, pp, lp, k, part, st);
            else if (m % 8 == 0) dispatch_nq<8>(p, codes, N, n, m, pp, lp, k, part, st);
            else if (m % 4 == 0) dispatch_nq<4>(p, codes, N, n, m, pp, lp, k, part, st);
            else dispatch_nq<1>(p, codes, N, n, m, pp, lp, k, part, st);
            WISE_LAUNCH_CHECK("pqflat_scan_kernel");
        }
        if (int rc = launch_merge_keys(part, n > 0 ? p.grid : 0, p.nq, p.nq, k, reinterpret_cast<const long long*>(ids), (long long)id_base,
                                       outD, reinterpret_cast<long long*>(outI), q0, st))
            return rc;
        q0 += p.nq;
    }
    return WISE_OK;
}

}  // namespace pq_flat
}  // namespace wise

using namespace wise;
using namespace wise::pq_flat;

extern "C" size_t wise_pqflat_topk_workspace_bytes(int64_t N, int m, int nq, int k) {
    if (!shape_ok(N, m, nq, k)) return 0;
    return part_bytes(N, m, nq > 0 ? nq : 1, k);
}

extern "C" int wise_pqflat_topk(const uint8_t* codes, int64_t N, int m, const float* lut, int nq, int k, const int64_t* ids, int64_t id_base,
                                float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream) {
    return topk_impl("pqflat_topk", codes, N, m, nullptr, N, false, lut, nq, k, ids, id_base, outD, outI, workspace, workspace_bytes, stream);
}

extern "C" int wise_pqflat_topk_pos(const uint8_t* codes, int64_t N, int m, const int64_t* pos, int64_t n_pos, const float* lut, int nq,
                                    int k, const int64_t* ids, int64_t id_base, float* outD, int64_t* outI, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    return topk_impl("pqflat_topk_pos", codes, N, m, pos, n_pos, true, lut, nq, k, ids, id_base, outD, outI, workspace, workspace_bytes,
                     stream);
}

extern "C" int wise_pqflat_decode(const uint8_t* codes, int64_t N, const int64_t* pos, int rows, const float* codebooks, int d, int m,
                                  float* out, void* stream) {
    if (d < 2 || m < 1 || m > 128 || d % m || (d / m) % 2 || d / m > 96) {
        set_error("pqflat_decode: d=%d m=%d unsupported (8-bit codes; d %% m == 0, m <= 128, d / m even in [2, 96])", d, m);
        return WISE_E_UNSUPPORTED;
    }
    WISE_CHECK_ARG(N >= 0 && rows >= 0 && codebooks && (N == 0 || codes) && (rows == 0 || (pos && out)), "pqflat_decode: bad argument");
    if (rows == 0) return WISE_OK;
    hipLaunchKernelGGL(pqflat_decode_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, codes, (long long)N, (const long long*)pos,
                       codebooks, d, m, out);
    WISE_LAUNCH_CHECK("pqflat_decode_kernel");
    return WISE_OK;
}

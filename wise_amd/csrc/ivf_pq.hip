// HP-2: IndexIVFPQ — inverted lists of 8-bit product-quantizer codes (faiss IndexIVFPQ over IndexFlatIP, by_residual, inner product).
// A row x of list l is kept as m bytes: its residual r = x - c_l cut into m sub-vectors of dsub = d / m floats, each replaced by
// the number of its nearest (L2) codeword among the 256 of its sub-space.  The codebooks [m][256][dsub] are shared by all lists.
//   wise_pq_residuals   r = x - c[assign]
//   wise_pq_encode      nearest codeword per sub-vector: argmax_c (r_j . cb_jc - 1/2 ||cb_jc||^2), ties to the lowest c; the
//                       assignment step of training and the encoder of add_with_ids.  256 d MACs per row on the VALU; the
//                       sub-space's codebook (<= 96 KiB) and a tile of 128 sub-vectors go through LDS
//   wise_pq_update      one Lloyd update: per (j, c) the mean of the assigned sub-vectors, summed in row order by one wave (the
//                       same bits run after run); an empty codeword keeps its value
//   wise_pq_lut         per query the table lut[j][c] = q_j . cb_jc (inner product: the table does not depend on the list)
//   wise_pq_bias        q . c_l for the probed lists: the one term of a row's score that depends on its list
//   wise_ivfpq_scan     THE HOT PATH: score(row) = bias + sum_j lut[j][code_j], added in that order in fp32, top-k per query
//   wise_pq_gather_codes  the grouping by list of add_with_ids (rows of m bytes)
//   wise_pq_find / wise_pq_decode   reconstruct_batch: id -> position, then c_l + concat_j cb[j][code_j]
// The scan reads m bytes per row where wise_ivf_scan_f32 reads 4 d.  A list is ~300 rows, i.e. less than the query's table
// (m KiB), so a block per (query, probe) would spend its time loading tables: a block loads its query's table into LDS once
// and walks a contiguous group of that query's probes, its waves taking 64 rows at a time, one lane per row.  Table reads are
// random ds_read_b32 (bank conflicts are inherent to the method).  Selection is the flat scan's: sortable (score, position)
// keys against per-wave threshold lists, folded per block, then merge_keys_kernel.
//   wise_ivfpq_scan_local  the same scan on ONE RANK's slice of a list-major index sharded across GPUs (list_off clipped to the
//                       slice: about nprobe / W of a query's probes hold rows there).  compact_probes_bias_kernel (probe_compact.h) keeps those
//                       probes and their bias, in probe order, and from the kept count fixes how many probe groups the query
//                       uses; a block past that number returns before it touches the table, the others share the kept probes
//                       evenly.  Same kernel body as the whole-index scan (pq_scan_kernel<VEC, true>).
#include "probe_compact.h"

namespace wise {
namespace ivf_pq {

constexpr int KSUB = 256;                 // codewords per sub-space (nbits = 8)
constexpr int ENC_ROWS = 128;             // rows per workgroup of the encoder
constexpr int LDS_MAX = 160 * 1024;       // one workgroup may take the whole CU's LDS

__global__ __launch_bounds__(256) void residuals_kernel(const float* __restrict__ x, const float* __restrict__ cent,
                                                        const long long* __restrict__ assign, long long n, int d, int nlist,
                                                        float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    long long l = assign[row];
    if (l < 0 || l >= nlist) l = 0;           // (validated by the caller; stay in bounds whatever comes)
    const float* xr = x + (size_t)row * d;
    const float* cr = cent + (size_t)l * d;
    for (int c = lane; c < d; c += 64) out[(size_t)row * d + c] = xr[c] - cr[c];
}

// block = (tile of ENC_ROWS rows, sub-space j); thread = one row.  LDS: cb [256][dsub], half norms [256], the tile's sub-vectors
// transposed rs [dsub][ENC_ROWS] (thread t reads rs[i][t]: conflict-free; cb reads are broadcasts).
__global__ __launch_bounds__(ENC_ROWS) void encode_kernel(const float* __restrict__ resid, const float* __restrict__ cbs, long long n,
                                                          int d, int m, unsigned char* __restrict__ codes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int dsub = d / m, j = blockIdx.y, t = threadIdx.x;
    float* cb = reinterpret_cast<float*>(smem);
    float* half = cb + (size_t)KSUB * dsub;
    float* rs = half + KSUB;
    const float* src = cbs + (size_t)j * KSUB * dsub;
    for (int i = t; i < KSUB * dsub; i += ENC_ROWS) cb[i] = src[i];
    const long long row0 = (long long)blockIdx.x * ENC_ROWS;
    for (int i = t; i < ENC_ROWS * dsub; i += ENC_ROWS) {
        const int r = i / dsub, c = i - r * dsub;
        rs[c * ENC_ROWS + r] = row0 + r < n ? resid[(size_t)(row0 + r) * d + (size_t)j * dsub + c] : 0.f;
    }
    __syncthreads();
    for (int c = t; c < KSUB; c += ENC_ROWS) {
        float q = 0.f;
        for (int i = 0; i < dsub; ++i) q = fmaf(cb[c * dsub + i], cb[c * dsub + i], q);
        half[c] = 0.5f * q;
    }
    __syncthreads();
    float best = -INFINITY;
    int bi = 0;
    for (int c = 0; c < KSUB; c += 4) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;          // four index-ordered chains share each read of r
        const float* c0 = cb + (size_t)c * dsub;
        for (int i = 0; i < dsub; ++i) {
            const float r = rs[i * ENC_ROWS + t];
            a0 = fmaf(r, c0[i], a0);
            a1 = fmaf(r, c0[dsub + i], a1);
            a2 = fmaf(r, c0[2 * dsub + i], a2);
            a3 = fmaf(r, c0[3 * dsub + i], a3);
        }
        a0 -= half[c]; a1 -= half[c + 1]; a2 -= half[c + 2]; a3 -= half[c + 3];
        if (a0 > best) { best = a0; bi = c; }
        if (a1 > best) { best = a1; bi = c + 1; }
        if (a2 > best) { best = a2; bi = c + 2; }
        if (a3 > best) { best = a3; bi = c + 3; }
    }
    if (row0 + t < n) codes[(size_t)(row0 + t) * m + j] = (unsigned char)bi;
}

// block = one wave = codeword (j, c): walk the rows 64 at a time, add the matching sub-vectors in ascending row order
// (lane = coordinate, two per lane when dsub > 64)
__global__ __launch_bounds__(64) void update_kernel(const float* __restrict__ resid, const unsigned char* __restrict__ codes, long long n,
                                                    int d, int m, const float* __restrict__ cb_in, float* __restrict__ cb_out) {
    const int dsub = d / m, c = blockIdx.x, j = blockIdx.y, lane = threadIdx.x;
    float s0 = 0.f, s1 = 0.f;
    unsigned count = 0;
    for (long long i0 = 0; i0 < n; i0 += 64) {
        const long long i = i0 + lane;
        const bool hit = i < n && codes[(size_t)i * m + j] == (unsigned char)c;
        unsigned long long mask = __ballot(hit);
        count += (unsigned)__popcll(mask);
        while (mask) {
            const int b = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const float* r = resid + (size_t)(i0 + b) * d + (size_t)j * dsub;
            if (lane < dsub) s0 += r[lane];
            if (lane + 64 < dsub) s1 += r[lane + 64];
        }
    }
    const size_t o = ((size_t)j * KSUB + c) * dsub;
    if (lane < dsub) cb_out[o + lane] = count ? s0 / (float)count : cb_in[o + lane];
    if (lane + 64 < dsub) cb_out[o + lane + 64] = count ? s1 / (float)count : cb_in[o + lane + 64];
}

// block = (sub-space j, query); thread = codeword
__global__ __launch_bounds__(KSUB) void lut_kernel(const float* __restrict__ Q, const float* __restrict__ cbs, int d, int m,
                                                   float* __restrict__ lut) {
    __shared__ float qs[96];
    const int dsub = d / m, j = blockIdx.x, q = blockIdx.y, c = threadIdx.x;
    if (c < dsub) qs[c] = Q[(size_t)q * d + (size_t)j * dsub + c];
    __syncthreads();
    const float* cb = cbs + ((size_t)j * KSUB + c) * dsub;
    float a = 0.f;
    for (int i = 0; i < dsub; ++i) a = fmaf(qs[i], cb[i], a);
    lut[((size_t)q * m + j) * KSUB + c] = a;
}

// one wave per (query, probe): q . c_l, lane-strided fmaf chains and a butterfly sum; a skipped probe (< 0) gets 0
__global__ __launch_bounds__(256) void bias_kernel(const float* __restrict__ Q, const float* __restrict__ cent,
                                                   const long long* __restrict__ probes, long long total, int nprobe, int nlist,
                                                   int d, float* __restrict__ bias) {
    const int lane = threadIdx.x & 63;
    const long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= total) return;
    const long long l = probes[e];
    float a = 0.f;
    if (l >= 0 && l < nlist) {
        const float* q = Q + (size_t)(e / nprobe) * d;
        const float* c = cent + (size_t)l * d;
        for (int i = lane; i < d; i += 64) a = fmaf(q[i], c[i], a);
    }
    a = wave_sum(a);
    if (lane == 0) bias[e] = a;
}

// VEC = bytes per load of a row's codes (m % VEC == 0, rows are VEC-aligned because the base is 16-byte aligned)
template <int VEC>
__device__ __forceinline__ float pq_row_score(const unsigned char* __restrict__ row, int m, const float* __restrict__ tab, float acc) {
    if constexpr (VEC == 1) {
        for (int j = 0; j < m; ++j) acc += tab[j * KSUB + row[j]];
    } else {
        using word_t = unsigned __attribute__((ext_vector_type(VEC / 4)));
        for (int j0 = 0; j0 < m; j0 += VEC) {
            const word_t w = __builtin_nontemporal_load(reinterpret_cast<const word_t*>(row + j0));
#pragma unroll
            for (int b = 0; b < VEC; ++b) {
                const unsigned word = w[b >> 2];
                acc += tab[(j0 + b) * KSUB + ((word >> (8 * (b & 3))) & 255u)];      // j ascending: the contract's order
            }
        }
    }
    return acc;
}

// The least number of kept probes a probe group of the rank-local scan must have before a further group is opened.
// plan_scan never launches more than about two blocks per CU, so on a device that runs nothing else a further group costs no
// time, while a longer share lengthens the slowest block of the launch, which is what a caller waits for; what a larger share
// saves is table traffic (m KiB per group) only.  1 = a group exists exactly when it has a probe with rows to scan: the
// table is then copied once per kept probe at most — nprobe / W times instead of nprobe times — and the slowest block never
// has more kept probes than the slowest block of the whole-index kernel run over the clipped offsets.
constexpr int LOCAL_MIN_SHARE = 1;      // min_share of compact_probes_bias_kernel (probe_compact.h)

// grid (G, nq): block (g, q) scans probes [g * per, (g + 1) * per) of query q; its k keys go to part[g][q][:]
// LOCAL (wise_ivfpq_scan_local): probes / bias are the compacted ones, count[q] of them live, dealt evenly to used[q] groups;
// a block past used[q] returns BEFORE the table copy (its slot of part is never read: the merge folds used[q] lists)
// SEL (wise_ivfpq_scan_sel): only the rows whose bit of `keep` is set are scored and offered — the score of such a row is the
// unfiltered scan's, bit for bit; a wave whose 64 rows are all clear goes on to its next 64 (offer's ballot: wave-uniform)
template <int VEC, bool LOCAL, bool SEL = false>
__global__ __launch_bounds__(256) void pq_scan_kernel(const unsigned char* __restrict__ codes, const long long* __restrict__ list_off,
                                                      int nlist, const float* __restrict__ lut, const long long* __restrict__ probes,
                                                      const float* __restrict__ bias, int nprobe, int per, int m, int k, int cap,
                                                      u64* __restrict__ part, const int* __restrict__ count,
                                                      const int* __restrict__ used, const unsigned* __restrict__ keep = nullptr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int q = blockIdx.y, g = blockIdx.x;
    int p0, p1;
    if constexpr (LOCAL) {
        const int groups = used[q];                                         // block-uniform
        if (g >= groups) return;
        const long long np = count[q];
        p0 = (int)(np * g / groups);
        p1 = (int)(np * (g + 1) / groups);
    } else {
        p0 = g * per;
        p1 = p0 + per < nprobe ? p0 + per : nprobe;
    }
    float* tab = reinterpret_cast<float*>(smem);
    u64* lists = reinterpret_cast<u64*>(smem + (size_t)m * KSUB * 4);
    {
        const float4* src = reinterpret_cast<const float4*>(lut + (size_t)q * m * KSUB);
        float4* dst = reinterpret_cast<float4*>(tab);
        for (int i = threadIdx.x; i < m * (KSUB / 4); i += blockDim.x) dst[i] = src[i];
    }
    WaveList wl;
    wl.init(lists + (size_t)wave * cap, cap, k, lane);
    __syncthreads();
    for (int p = p0; p < p1; ++p) {
        const long long l = probes[(size_t)q * nprobe + p];
        if (l < 0 || l >= nlist) continue;                              // block-uniform
        const float b = bias[(size_t)q * nprobe + p];
        const long long lo = list_off[l], hi = list_off[l + 1];
        for (long long r0 = lo + wave * 64; r0 < hi; r0 += (long long)nwaves * 64) {      // wave-uniform
            const long long row = r0 + lane;
            bool live = row < hi;
            if constexpr (SEL) live = live && ((keep[row >> 5] >> (row & 31)) & 1u) != 0;
            float s = b;
            if (live) s = pq_row_score<VEC>(codes + (size_t)row * m, m, tab, b);
            const u64 key = make_key(s, (unsigned)row);
            wl.offer(live && key > wl.tau, key, lane);
        }
    }
    wl.compact(lane);
    __syncthreads();
    if (wave == 0) {
        for (int w = 1; w < nwaves; ++w) {
            const u64* other = lists + (size_t)w * cap;
            for (int i0 = 0; i0 < k; i0 += 64) {
                const int i = i0 + lane;
                const u64 key = i < k ? other[i] : 0;
                wl.offer(key != 0 && key > wl.tau, key, lane);
            }
        }
        wl.compact(lane);
        u64* dst = part + ((size_t)g * gridDim.y + q) * k;
        for (int i = lane; i < k; i += 64) dst[i] = wl.buf[i];
    }
}

// out[i][:] = codes[idx[i]][:] (rows of m bytes): the grouping by list of add_with_ids
__global__ __launch_bounds__(256) void gather_codes_kernel(const unsigned char* __restrict__ codes, const long long* __restrict__ idx,
                                                           long long total, int m, unsigned char* __restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long i = e / m;
    out[e] = codes[(size_t)idx[i] * m + (e - i * m)];
}

// pos[i] = position of query_ids[i] in ids (the highest, if it occurs more than once), -1 when absent
__global__ __launch_bounds__(256) void find_kernel(const long long* __restrict__ ids, long long N, const long long* __restrict__ qids,
                                                   long long* __restrict__ pos) {
    const long long row = row_of_id(ids, 0, N, qids[blockIdx.x]);
    if (threadIdx.x == 0) pos[blockIdx.x] = row;
}

// out[i][:] = c_l + concat_j cb[j][codes[pos[i]][j]], l = the list that holds position pos[i]; NaN when pos[i] is out of range
__global__ __launch_bounds__(256) void decode_kernel(const unsigned char* __restrict__ codes, long long N, const long long* __restrict__ pos,
                                                     const long long* __restrict__ list_off, int nlist, const float* __restrict__ cent,
                                                     const float* __restrict__ cbs, int d, int m, float* __restrict__ out) {
    const int dsub = d / m;
    const long long p = pos[blockIdx.x];
    float* o = out + (size_t)blockIdx.x * d;
    if (p < 0 || p >= N) {
        for (int c = threadIdx.x; c < d; c += blockDim.x) o[c] = __builtin_nanf("");
        return;
    }
    int a = 0, b = nlist;                        // the last list whose offset is <= p (empty lists share offsets: skip them)
    while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if (list_off[mid] <= p) a = mid; else b = mid;
    }
    const float* cr = cent + (size_t)a * d;
    const unsigned char* code = codes + (size_t)p * m;
    for (int c = threadIdx.x; c < d; c += blockDim.x) {
        const int j = c / dsub, t = c - j * dsub;
        o[c] = cr[c] + cbs[((size_t)j * KSUB + code[j]) * dsub + t];
    }
}

static bool pq_shape_ok(int d, int m) {
    if (d < 2 || m < 1 || m > 128 || d % m) return false;
    const int dsub = d / m;
    return dsub >= 2 && dsub <= 96 && dsub % 2 == 0;
}

struct ScanShape {
    int groups, per, waves, cap;
    size_t lds;
};
// G probe groups per query so that nq * G is about two blocks per CU; as many waves as the LDS left by the table allows
static bool plan_scan(int nq, int nprobe, int k, int m, ScanShape* s) {
    if (nq < 1 || nprobe < 1 || nprobe > 2048 || k < 1 || k > 2048 || m < 1 || m > 128) return false;
    int G = (512 + nq - 1) / nq;
    if (G > nprobe) G = nprobe;
    s->per = (nprobe + G - 1) / G;
    s->groups = (nprobe + s->per - 1) / s->per;
    s->cap = topk_list_cap(k);
    const size_t tab = (size_t)m * KSUB * 4;
    s->waves = 4;
    while (s->waves > 1 && tab + (size_t)s->waves * s->cap * 8 > (size_t)LDS_MAX) s->waves >>= 1;
    s->lds = tab + (size_t)s->waves * s->cap * 8;
    return s->lds <= (size_t)LDS_MAX;
}

template <int VEC, bool LOCAL>
static void launch_pq_scan(const ScanShape& s, int nq, const unsigned char* codes, const long long* list_off, int nlist, const float* lut,
                           const long long* probes, const float* bias, int nprobe, int m, int k, u64* part, hipStream_t st,
                           const int* count = nullptr, const int* used = nullptr, const unsigned* keep = nullptr) {
    auto kern = pq_scan_kernel<VEC, LOCAL>;
    if constexpr (!LOCAL) {
        if (keep) kern = pq_scan_kernel<VEC, false, true>;
    }
    if (s.lds > 48 * 1024) raise_lds_limit(reinterpret_cast<const void*>(kern), (int)s.lds);
    hipLaunchKernelGGL(kern, dim3(s.groups, nq), dim3(s.waves * 64), s.lds, st, codes, list_off, nlist, lut, probes, bias, nprobe,
                       s.per, m, k, s.cap, part, count, used, keep);
}

// Workspace of the rank-local scan (LocalWorkspace, probe_compact.h): the keys are [groups][nq][k]
static size_t local_part_bytes(const ScanShape& s, int nq, int k) { return align_up((size_t)s.groups * nq * k * sizeof(u64), 256); }

}  // namespace ivf_pq
}  // namespace wise

using namespace wise;
using namespace wise::ivf_pq;

#define PQ_CHECK_SHAPE(what)                                                                                              \
    do {                                                                                                                  \
        if (!pq_shape_ok(d, m)) {                                                                                         \
            set_error(what ": d=%d m=%d unsupported (8-bit codes; d %% m == 0, m <= 128, d / m even in [2, 96])", d, m);  \
            return WISE_E_UNSUPPORTED;                                                                                    \
        }                                                                                                                 \
    } while (0)

extern "C" int wise_pq_residuals(const float* x, const float* centroids, const int64_t* assign, int64_t n, int d, int nlist, float* out,
                                 void* stream) {
    WISE_CHECK_ARG(n >= 0 && d > 0 && nlist > 0 && (n == 0 || (x && centroids && assign && out)), "pq_residuals: bad argument");
    if (n == 0) return WISE_OK;
    hipLaunchKernelGGL(residuals_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, centroids,
                       (const long long*)assign, (long long)n, d, nlist, out);
    WISE_LAUNCH_CHECK("pq residuals_kernel");
    return WISE_OK;
}

extern "C" int wise_pq_encode(const float* resid, const float* codebooks, int64_t n, int d, int m, uint8_t* codes, void* stream) {
    PQ_CHECK_SHAPE("pq_encode");
    WISE_CHECK_ARG(n >= 0 && n < (1ll << 31) * ENC_ROWS && codebooks && (n == 0 || (resid && codes)), "pq_encode: bad argument");
    if (n == 0) return WISE_OK;
    const int dsub = d / m;
    const size_t lds = ((size_t)KSUB * dsub + KSUB + (size_t)ENC_ROWS * dsub) * 4;
    if (lds > 48 * 1024) raise_lds_limit(reinterpret_cast<const void*>(encode_kernel), (int)lds);
    hipLaunchKernelGGL(encode_kernel, dim3((unsigned)((n + ENC_ROWS - 1) / ENC_ROWS), m), dim3(ENC_ROWS), lds, (hipStream_t)stream,
                       resid, codebooks, (long long)n, d, m, codes);
    WISE_LAUNCH_CHECK("pq encode_kernel");
    return WISE_OK;
}

extern "C" int wise_pq_update(const float* resid, const uint8_t* codes, int64_t n, int d, int m, const float* codebooks_in,
                              float* codebooks_out, void* stream) {
    PQ_CHECK_SHAPE("pq_update");
    WISE_CHECK_ARG(n >= 0 && codebooks_in && codebooks_out && codebooks_in != codebooks_out && (n == 0 || (resid && codes)),
                   "pq_update: bad argument (codebooks_out must not alias codebooks_in)");
    hipLaunchKernelGGL(update_kernel, dim3(KSUB, m), dim3(64), 0, (hipStream_t)stream, resid, codes, (long long)n, d, m, codebooks_in,
                       codebooks_out);
    WISE_LAUNCH_CHECK("pq update_kernel");
    return WISE_OK;
}

extern "C" int wise_pq_lut(const float* Q, const float* codebooks, int nq, int d, int m, float* lut, void* stream) {
    PQ_CHECK_SHAPE("pq_lut");
    WISE_CHECK_ARG(nq >= 0 && nq <= 65535 && codebooks && (nq == 0 || (Q && lut)), "pq_lut: bad argument (nq <= 65535)");
    if (nq == 0) return WISE_OK;
    hipLaunchKernelGGL(lut_kernel, dim3(m, nq), dim3(KSUB), 0, (hipStream_t)stream, Q, codebooks, d, m, lut);
    WISE_LAUNCH_CHECK("pq lut_kernel");
    return WISE_OK;
}

extern "C" int wise_pq_bias(const float* Q, const float* centroids, const int64_t* probes, int nq, int nprobe, int nlist, int d,
                            float* bias, void* stream) {
    WISE_CHECK_ARG(nq >= 0 && nprobe >= 1 && nlist >= 1 && d >= 1 && centroids && (nq == 0 || (Q && probes && bias)),
                   "pq_bias: bad argument");
    if (nq == 0) return WISE_OK;
    const long long total = (long long)nq * nprobe;
    hipLaunchKernelGGL(bias_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, (hipStream_t)stream, Q, centroids,
                       (const long long*)probes, total, nprobe, nlist, d, bias);
    WISE_LAUNCH_CHECK("pq bias_kernel");
    return WISE_OK;
}

extern "C" size_t wise_ivfpq_scan_workspace_bytes(int nq, int nprobe, int k, int m) {
    ScanShape s;
    if (!plan_scan(nq, nprobe, k, m, &s)) return 0;
    return align_up((size_t)s.groups * nq * k * sizeof(u64), 256);
}

// wise_ivfpq_scan and, with keep, wise_ivfpq_scan_sel
static int pq_scan_impl(const char* what, const uint8_t* codes, int64_t N, int m, const int64_t* list_off, int nlist, const int64_t* ids,
                        const float* lut, int nq, const int64_t* probes, const float* bias, int nprobe, int k, float* outD,
                        int64_t* outI, void* workspace, size_t workspace_bytes, void* stream, const uint32_t* keep) {
    ScanShape s;
    if (!plan_scan(nq, nprobe, k, m, &s) || nq > 65535) {
        set_error("%s: nq=%d nprobe=%d k=%d m=%d unsupported (nq <= 65535, nprobe <= 2048, k <= 2048, m <= 128)", what, nq, nprobe, k, m);
        return WISE_E_UNSUPPORTED;
    }
    WISE_CHECK_ARG(nlist >= 1 && N >= 0 && N < 0xFFFFFFFFll, "%s: N=%lld nlist=%d out of range", what, (long long)N, nlist);
    WISE_CHECK_ARG(lut && probes && bias && outD && outI && list_off && (codes || N == 0), "%s: null pointer", what);
    WISE_CHECK_ARG(((uintptr_t)codes & 15) == 0 && ((uintptr_t)lut & 15) == 0, "%s: codes and lut must be 16-byte aligned", what);
    const size_t need = wise_ivfpq_scan_workspace_bytes(nq, nprobe, k, m);
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace %zu < %zu bytes", what, workspace_bytes, need);
        return WISE_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    u64* part = reinterpret_cast<u64*>(workspace);
    const long long* lo = reinterpret_cast<const long long*>(list_off);
    const long long* pr = reinterpret_cast<const long long*>(probes);
    if (m % 16 == 0) launch_pq_scan<16, false>(s, nq, codes, lo, nlist, lut, pr, bias, nprobe, m, k, part, st, nullptr, nullptr, keep);
    else if (m % 8 == 0) launch_pq_scan<8, false>(s, nq, codes, lo, nlist, lut, pr, bias, nprobe, m, k, part, st, nullptr, nullptr, keep);
    else if (m % 4 == 0) launch_pq_scan<4, false>(s, nq, codes, lo, nlist, lut, pr, bias, nprobe, m, k, part, st, nullptr, nullptr, keep);
    else launch_pq_scan<1, false>(s, nq, codes, lo, nlist, lut, pr, bias, nprobe, m, k, part, st, nullptr, nullptr, keep);
    WISE_LAUNCH_CHECK("pq_scan_kernel");
    return merge_lists_launch(part, s.groups, nq, k, reinterpret_cast<const long long*>(ids), outD, reinterpret_cast<long long*>(outI), st);
}

extern "C" int wise_ivfpq_scan(const uint8_t* codes, int64_t N, int m, const int64_t* list_off, int nlist, const int64_t* ids,
                               const float* lut, int nq, const int64_t* probes, const float* bias, int nprobe, int k, float* outD,
                               int64_t* outI, void* workspace, size_t workspace_bytes, void* stream) {
    return pq_scan_impl("ivfpq_scan", codes, N, m, list_off, nlist, ids, lut, nq, probes, bias, nprobe, k, outD, outI, workspace,
                        workspace_bytes, stream, nullptr);
}

extern "C" int wise_ivfpq_scan_sel(const uint8_t* codes, int64_t N, int m, const int64_t* list_off, int nlist, const int64_t* ids,
                                   const float* lut, int nq, const int64_t* probes, const float* bias, int nprobe, int k,
                                   const uint32_t* keep, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    WISE_CHECK_ARG(keep || N == 0, "ivfpq_scan_sel: null bitmap");
    return pq_scan_impl("ivfpq_scan_sel", codes, N, m, list_off, nlist, ids, lut, nq, probes, bias, nprobe, k, outD, outI, workspace,
                        workspace_bytes, stream, keep);
}

extern "C" size_t wise_ivfpq_scan_local_workspace_bytes(int nq, int nprobe, int k, int m) {
    ScanShape s;
    if (!plan_scan(nq, nprobe, k, m, &s) || nq > 65535) return 0;
    return LocalWorkspace::bytes(local_part_bytes(s, nq, k), nq, nprobe);
}

extern "C" int wise_ivfpq_scan_local(const uint8_t* codes, int64_t N, int m, const int64_t* list_off, int nlist, const int64_t* ids,
                                     const float* lut, int nq, const int64_t* probes, const float* bias, int nprobe, int k,
                                     int64_t pos_base, float* outD, int64_t* outI, int32_t* probe_count, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    ScanShape s;
    if (!plan_scan(nq, nprobe, k, m, &s) || nq > 65535) {
        set_error("ivfpq_scan_local: nq=%d nprobe=%d k=%d m=%d unsupported (nq <= 65535, nprobe <= 2048, k <= 2048, m <= 128)", nq, nprobe, k,
                  m);
        return WISE_E_UNSUPPORTED;
    }
    WISE_CHECK_ARG(nlist >= 1 && N >= 0 && N < 0xFFFFFFFFll && pos_base >= 0, "ivfpq_scan_local: N=%lld nlist=%d pos_base=%lld out of range",
                   (long long)N, nlist, (long long)pos_base);
    WISE_CHECK_ARG(lut && probes && bias && outD && outI && list_off && (codes || N == 0), "ivfpq_scan_local: null pointer");
    WISE_CHECK_ARG(((uintptr_t)codes & 15) == 0 && ((uintptr_t)lut & 15) == 0, "ivfpq_scan_local: codes and lut must be 16-byte aligned");
    const size_t need = wise_ivfpq_scan_local_workspace_bytes(nq, nprobe, k, m);
    if (!workspace || workspace_bytes < need) {
        set_error("ivfpq_scan_local: workspace %zu < %zu bytes", workspace_bytes, need);
        return WISE_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const LocalWorkspace lw = LocalWorkspace::carve(workspace, local_part_bytes(s, nq, k), nq, nprobe, probe_count);
    const long long* lo = reinterpret_cast<const long long*>(list_off);
    hipLaunchKernelGGL(compact_probes_bias_kernel<true>, dim3(nq), dim3(64), 0, st, reinterpret_cast<const long long*>(probes), bias, nprobe, lo,
                       nlist, s.groups, LOCAL_MIN_SHARE, lw.live, lw.lbias, lw.count, lw.used);
    WISE_LAUNCH_CHECK("compact_probes_bias_kernel");
    if (m % 16 == 0) launch_pq_scan<16, true>(s, nq, codes, lo, nlist, lut, lw.live, lw.lbias, nprobe, m, k, lw.part, st, lw.count, lw.used);
    else if (m % 8 == 0) launch_pq_scan<8, true>(s, nq, codes, lo, nlist, lut, lw.live, lw.lbias, nprobe, m, k, lw.part, st, lw.count, lw.used);
    else if (m % 4 == 0) launch_pq_scan<4, true>(s, nq, codes, lo, nlist, lut, lw.live, lw.lbias, nprobe, m, k, lw.part, st, lw.count, lw.used);
    else launch_pq_scan<1, true>(s, nq, codes, lo, nlist, lut, lw.live, lw.lbias, nprobe, m, k, lw.part, st, lw.count, lw.used);
    WISE_LAUNCH_CHECK("pq_scan_kernel<local>");
    // keys carry local rows; without ids the merge writes pos_base + row, the row's position in the whole array
    return merge_lists_launch(lw.part, s.groups, nq, k, reinterpret_cast<const long long*>(ids), outD, reinterpret_cast<long long*>(outI),
                              st, lw.used, (long long)pos_base);
}

extern "C" int wise_pq_gather_codes(const uint8_t* codes, const int64_t* idx, int64_t n, int m, uint8_t* out, void* stream) {
    WISE_CHECK_ARG(n >= 0 && m >= 1 && m <= 128 && n < (1ll << 32) && (n == 0 || (codes && idx && out)), "pq_gather_codes: bad argument");
    if (n == 0) return WISE_OK;
    const long long total = (long long)n * m;
    hipLaunchKernelGGL(gather_codes_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, codes,
                       (const long long*)idx, total, m, out);
    WISE_LAUNCH_CHECK("pq gather_codes_kernel");
    return WISE_OK;
}

extern "C" int wise_pq_find(const int64_t* ids, int64_t N, const int64_t* query_ids, int n, int64_t* pos, void* stream) {
    WISE_CHECK_ARG(N >= 0 && n >= 0 && (N == 0 || ids) && (n == 0 || (query_ids && pos)), "pq_find: bad argument");
    if (n == 0) return WISE_OK;
    hipLaunchKernelGGL(find_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, (const long long*)ids, (long long)N,
                       (const long long*)query_ids, (long long*)pos);
    WISE_LAUNCH_CHECK("pq find_kernel");
    return WISE_OK;
}

extern "C" int wise_pq_decode(const uint8_t* codes, int64_t N, const int64_t* pos, int rows, const int64_t* list_off, int nlist,
                              const float* centroids, const float* codebooks, int d, int m, float* out, void* stream) {
    PQ_CHECK_SHAPE("pq_decode");
    WISE_CHECK_ARG(N >= 0 && rows >= 0 && nlist >= 1 && list_off && centroids && codebooks && (N == 0 || codes) && (rows == 0 || (pos && out)),
                   "pq_decode: bad argument");
    if (rows == 0) return WISE_OK;
    hipLaunchKernelGGL(decode_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, codes, (long long)N, (const long long*)pos,
                       (const long long*)list_off, nlist, centroids, codebooks, d, m, out);
    WISE_LAUNCH_CHECK("pq decode_kernel");
    return WISE_OK;
}

// HP-2: IndexIVFSQ8 — inverted lists of 8-bit scalar-quantized rows (faiss IndexIVFScalarQuantizer over IndexFlatIP, QT_8bit,
// by_residual, inner product).  A row x of list l is kept as d bytes: its residual r = x - c_l, every dimension cut into 256
// bins of the range [vmin[i], vmin[i] + vdiff[i]] the trainer saw.  One range per dimension, shared by all lists; no codebooks
// and no per-query table.
//   wise_sq_train    per-dimension min and range of the training residuals (exact: order does not matter)
//   wise_sq_minmax   the same reduction as a running per-dimension minimum and maximum over chunks of rows (IndexSQ8bit)
//   wise_sq_encode   code_i = clamp(floor((r_i - vmin[i]) * (255 / vdiff[i])), 0, 255), evaluated in double
//   wise_sq_query    per query the weight row w[i] = q_i vdiff[i] / 255 and q0 = sum_i q_i (vmin[i] + vdiff[i] 0.5 / 255)
//   wise_sq_decode   reconstruct_batch: c_l + vmin + vdiff (code + 0.5) / 255 (faiss Codec8bit)
//   wise_ivfsq_scan  THE HOT PATH: score(row) = (bias + q0) + sum_i w[i] * code_i, top-k per query; wise_ivfsq_scan_sel the same
//                    under a bitmap over the list positions
// The scan reads d bytes per row where wise_ivf_scan_f32 reads 4 d.  One block per (query, probe), as the inverted-list form of
// ip_scan_kernel; four waves share the list.  A row is C = d / 16 chunks of 16 bytes and a lane always holds the same chunk
// c = lane % C of row lane / C of its wave-load, so the 16 weights of the chunk stay in registers: a 64-lane load carries
// RPL = 64 / C whole rows (four at d = 256, two at d = 512, one from d = 528 on; the lanes past RPL * C idle).  SQ_T loads are in
// flight per wave.  Per byte: one v_cvt_f32_ubyte and one v_fma_f32, i.e. 2 VALU lane-operations per byte against 64 per clock
// and CU — 32 B / clock / CU where HBM delivers about 13 (8 TB/s over 256 CUs at 2.4 GHz): the bound is HBM.
// THE SUMMATION ORDER (tests/ivfsq_ref.py restates it): lane (row, c) runs s = +0, s = fmaf(w[16 c + i], (float)code[16 c + i], s)
// for i = 0 .. 15; then for step = 1, 2, 4, ... < C every lane with c + step < C adds the value lane c + step held BEFORE the
// step (s_c = s_c + s_{c + step}); chunk 0 then holds the row's sum and score = (bias + q0) + s_0.  No packed f32 math.
// Selection is the flat scan's: sortable (score, position) keys, per-wave threshold lists, merge_keys_kernel.
//   wise_ivfsq_scan_local  the same scan on ONE RANK's slice of a list-major index sharded across GPUs (list_off clipped to the
//                    slice: about nprobe / W of a query's probes hold rows there).  compact_probes_bias_kernel (probe_compact.h)
//                    keeps those probes and their bias, in probe order; every kept probe is a probe group of its own, as every
//                    probe is a block of the whole scan, and a block past the kept count returns before it loads a weight.  A
//                    block's work on its list is sq_scan_list, the one body of all three kernels: a list cut by the slice scores
//                    its rows as the whole scan does, because a row's chunks and lanes depend on d alone and d % 16 == 0 keeps
//                    every row of a slice 16-byte aligned.
// IndexIVFSQfp16 (faiss QT_fp16) is the SAME kernels under a second codec (Codec16 below): a row is d IEEE binary16 values of its
// residual, nothing is trained, the query itself is the weight row and there is no q0.
//   wise_sq16_encode  halves = (binary16)r, round to nearest even, subnormals kept (the hardware conversion: numpy's cast)
//   wise_sq16_decode  reconstruct_batch: c_l + (float)h, one fp32 addition
//   wise_ivfsq16_scan / _scan_sel / _scan_local / wise_ivfsq16_range_*  score(row) = bias + sum_i Q[i] * (float)h_i, one
//                    v_fma_mix_f32 per element (1 VALU lane-operation per 2 bytes); chunk c = the row's 16-byte pieces c and c + C
// The SQ8 entry points instantiate the bodies with Codec8 and keep their arithmetic and their bits.
// The two codecs and sq_score_loads — the sum of the contract — live in sq_codec.h: the flat scan over binary16 rows (ip_sq16.hip,
// IndexSQfp16) scores with the same device code.
// IndexIVFFlatL2 (faiss IndexIVFFlat over IndexFlatL2, METRIC_L2: raw fp32 rows in the lists, no residual) is the SAME kernels under
// the flat L2 index's codec (CodecL2: the query is the weight row, s_0 is the squared distance) and the L2 sense of a score (SenseL2
// below): no bias, keys order -dist, a range hit is dist < radius, the sign flips back behind the merge.
//   wise_ivfl2_scan / _scan_sel / _scan_local / wise_ivfl2_range_*   a row's distance is wise_l2_topk_f32's, bit for bit
#include "probe_compact.h"
#include "range_common.h"
#include "sq_codec.h"

namespace wise {
namespace ivf_sq {

constexpr int MAX_D = 1024;

static bool sq_shape_ok(int d) { return d >= 16 && d <= MAX_D && d % 16 == 0; }

// THE SENSE of a list kernel's score, a static policy beside the codec (what flat_codec_scan.h's policies are to the flat scan): the
// row's value from its base and s_0, the score its key orders, and the range rule.  Nothing branches on it at run time.
//   SenseIP  the inner-product types: value = base + s_0 with base = the codec's (bias, q0) term; larger is better; hit: value > radius
//   SenseL2  IndexIVFFlatL2 over CodecL2: value = s_0, the squared distance itself (no bias is read: the pointer may be null); the
//            key orders -value (exact), so keys, ties and merges are the other types'; hit: value < radius.  FLIP: the merge's
//            output, scores and padding, is negated behind it (l2_flip_launch, l2_topk.hip)
struct SenseIP {
    static constexpr bool FLIP = false;
    template <class Codec>
    static __device__ __forceinline__ float base(const float* bias, size_t i, const float* q0, int qi) {
        return Codec::base(bias[i], q0, qi);
    }
    static __device__ __forceinline__ float value(float base, float s) { return base + s; }
    static __device__ __forceinline__ float key_score(float v) { return v; }
    static __device__ __forceinline__ bool range_hit(float v, float radius) { return v > radius; }
};
struct SenseL2 {
    static constexpr bool FLIP = true;
    template <class Codec>
    static __device__ __forceinline__ float base(const float*, size_t, const float*, int) { return 0.f; }
    static __device__ __forceinline__ float value(float, float s) { return s; }
    static __device__ __forceinline__ float key_score(float v) { return -v; }
    static __device__ __forceinline__ bool range_hit(float v, float radius) { return v < radius; }
};

// trained is used as 2 d ordered-unsigned cells while the reduction runs: min cells start at the largest key, max cells at 0
__global__ __launch_bounds__(256) void train_init_kernel(unsigned* __restrict__ cells, int d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 2 * d) cells[i] = i < d ? 0xFFFFFFFFu : 0u;
}

// block = (64 columns, a stride of rows); thread (column, row phase).  min / max are exact, so neither the order of the rows nor
// that of the atomics changes a bit of the result.
__global__ __launch_bounds__(256) void train_minmax_kernel(const float* __restrict__ r, long long n, int d, unsigned* __restrict__ mincells,
                                                           unsigned* __restrict__ maxcells) {
    __shared__ unsigned smin[4][64], smax[4][64];
    const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + cx;
    unsigned mn = 0xFFFFFFFFu, mx = 0u;
    if (col < d) {
        for (long long row = (long long)blockIdx.y * 4 + ry; row < n; row += (long long)gridDim.y * 4) {
            const unsigned o = f32_order(r[(size_t)row * d + col]);
            mn = o < mn ? o : mn;
            mx = o > mx ? o : mx;
        }
    }
    smin[ry][cx] = mn;
    smax[ry][cx] = mx;
    __syncthreads();
    if (ry == 0 && col < d) {
        for (int y = 1; y < 4; ++y) {
            mn = smin[y][cx] < mn ? smin[y][cx] : mn;
            mx = smax[y][cx] > mx ? smax[y][cx] : mx;
        }
        atomicMin(&mincells[col], mn);
        atomicMax(&maxcells[col], mx);
    }
}

__global__ __launch_bounds__(256) void train_finish_kernel(float* __restrict__ trained, int d) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d) return;
    const unsigned* cells = reinterpret_cast<const unsigned*>(trained);
    const float mn = f32_unorder(cells[i]), mx = f32_unorder(cells[d + i]);
    trained[i] = mn;
    trained[d + i] = mx - mn;
}

// wise_sq_minmax: lo / hi are used as ordered-unsigned cells while train_minmax_kernel runs.  open: the cells of what the arrays
// hold (accumulate) or of +3.4028235e38 / -3.4028235e38, the minimum and maximum of no rows; close: back to floats
__global__ __launch_bounds__(256) void minmax_open_kernel(float* __restrict__ lo, float* __restrict__ hi, int d, int accumulate) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d) return;
    const float a = accumulate ? lo[i] : 3.4028234663852886e38f, b = accumulate ? hi[i] : -3.4028234663852886e38f;
    reinterpret_cast<unsigned*>(lo)[i] = f32_order(a);
    reinterpret_cast<unsigned*>(hi)[i] = f32_order(b);
}
__global__ __launch_bounds__(256) void minmax_close_kernel(float* __restrict__ lo, float* __restrict__ hi, int d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d) return;
    lo[i] = f32_unorder(reinterpret_cast<const unsigned*>(lo)[i]);
    hi[i] = f32_unorder(reinterpret_cast<const unsigned*>(hi)[i]);
}

// thread = one value
__global__ __launch_bounds__(256) void encode_kernel(const float* __restrict__ r, const float* __restrict__ trained, long long total, int d,
                                                     unsigned char* __restrict__ codes) {
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int i = (int)(e % d);
    // in double: r - vmin is then exact (or as good as) and the bin is the one the real number falls into, so a value inside the
    // trained range decodes to within half a bin; in float the three roundings put values next to an edge into the wrong bin
    const double vmin = (double)trained[i], vdiff = (double)trained[d + i];
    const double inv = vdiff != 0.0 ? 255.0 / vdiff : 0.0;
    const double t = ((double)r[e] - vmin) * inv;
    double v = floor(t);
    v = v > 0.0 ? v : 0.0;                       // (a NaN lands here too)
    v = v < 255.0 ? v : 255.0;
    codes[e] = (unsigned char)(int)v;
}

// block = one wave = one query.  q0: lane l runs acc = +0, acc = acc + q_i * (vmin[i] + vdiff[i] * (0.5 / 255)) over i = l, l + 64,
// ... with every product and sum rounded on its own, then the butterfly wave_sum (xor 32, 16, ..., 1)
__global__ __launch_bounds__(64) void query_kernel(const float* __restrict__ Q, const float* __restrict__ trained, int d,
                                                   float* __restrict__ W, float* __restrict__ q0) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, q = blockIdx.x;
    const float inv255 = 1.0f / 255.0f, half255 = 0.5f / 255.0f;
    float acc = 0.f;
    for (int i = lane; i < d; i += 64) {
        const float qi = Q[(size_t)q * d + i], vmin = trained[i], vdiff = trained[d + i];
        const float qv = qi * vdiff;
        W[(size_t)q * d + i] = qv * inv255;
        const float h = vdiff * half255;
        const float t = vmin + h;
        const float p = qi * t;
        acc = acc + p;
    }
    acc = wave_sum(acc);
    if (lane == 0) q0[q] = acc;
}

// the decoders: the list that holds position p — the last list whose offset is <= p (empty lists share offsets: skip them)
__device__ __forceinline__ int list_of_position(const long long* __restrict__ list_off, int nlist, long long p) {
    int a = 0, b = nlist;
    while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if (list_off[mid] <= p) a = mid; else b = mid;
    }
    return a;
}

// out[i][:] = c_l + (vmin + ((code + 0.5) / 255) * vdiff), l = the list that holds position pos[i]; NaN when pos[i] is out of range
__global__ __launch_bounds__(256) void decode_kernel(const unsigned char* __restrict__ codes, long long N, const long long* __restrict__ pos,
                                                     const long long* __restrict__ list_off, int nlist, const float* __restrict__ cent,
                                                     const float* __restrict__ trained, int d, float* __restrict__ out) {
#pragma clang fp contract(off)
    const long long p = pos[blockIdx.x];
    float* o = out + (size_t)blockIdx.x * d;
    if (p < 0 || p >= N) {
        for (int c = threadIdx.x; c < d; c += blockDim.x) o[c] = __builtin_nanf("");
        return;
    }
    const float* cr = cent + (size_t)list_of_position(list_off, nlist, p) * d;
    const unsigned char* code = codes + (size_t)p * d;
    for (int c = threadIdx.x; c < d; c += blockDim.x) {
        const float xi = ((float)code[c] + 0.5f) / 255.0f;
        const float s = xi * trained[d + c];
        const float y = trained[c] + s;
        o[c] = cr[c] + y;
    }
}

// wise_sq16_encode: thread = one value; the conversion is the hardware's round-to-nearest-even with binary16 subnormals kept
__global__ __launch_bounds__(256) void encode16_kernel(const float* __restrict__ r, long long total, _Float16* __restrict__ halves) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e < total) halves[e] = (_Float16)r[e];
}

// wise_sq16_decode: out[i][:] = c_l + (float)halves[pos[i]][:], one fp32 addition; NaN when pos[i] is out of range
__global__ __launch_bounds__(256) void decode16_kernel(const _Float16* __restrict__ halves, long long N, const long long* __restrict__ pos,
                                                       const long long* __restrict__ list_off, int nlist, const float* __restrict__ cent,
                                                       int d, float* __restrict__ out) {
#pragma clang fp contract(off)
    const long long p = pos[blockIdx.x];
    float* o = out + (size_t)blockIdx.x * d;
    if (p < 0 || p >= N) {
        for (int c = threadIdx.x; c < d; c += blockDim.x) o[c] = __builtin_nanf("");
        return;
    }
    const float* cr = cent + (size_t)list_of_position(list_off, nlist, p) * d;
    const _Float16* h = halves + (size_t)p * d;
    for (int c = threadIdx.x; c < d; c += blockDim.x) o[c] = cr[c] + (float)h[c];
}

// One block's scan of the rows [lo, hi) of codes under the weight row wrow [d]: score = base + s_0 (SenseL2: -s_0); the k best keys go
// to dst.
// SEL: only the rows whose bit of `keep` is set are offered; a wave whose SQ_T loads hold no such row skips them (wave-uniform)
template <class Codec, bool SEL, class Sense = SenseIP>
__device__ __forceinline__ void sq_scan_list(const unsigned char* __restrict__ codes, long long lo, long long hi,
                                             const float* __restrict__ wrow, float base, int d, int k, int cap, u64* __restrict__ dst,
                                             const unsigned* __restrict__ keep) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C = d >> 4, RPL = 64 / C;
    const int sub = lane / C, c = lane - sub * C;
    const bool active = sub < RPL;
    float4 w[4];
    Codec::weights(wrow, d, c, w);

    WaveList wl;
    wl.init(reinterpret_cast<u64*>(smem) + (size_t)wave * cap, cap, k, lane);

    const long long ngroups = (hi - lo + RPL - 1) / RPL;                            // groups of RPL rows = wave-loads
    for (long long g = (long long)wave * SQ_T; g < ngroups; g += 4 * SQ_T) {       // wave-uniform
        long long row[SQ_T];
        bool live[SQ_T];
        bool any = false;
#pragma unroll
        for (int t = 0; t < SQ_T; ++t) {
            row[t] = lo + (g + t) * RPL + sub;
            live[t] = active && row[t] < hi;
            if constexpr (SEL) live[t] = live[t] && ((keep[row[t] >> 5] >> (row[t] & 31)) & 1u) != 0;
            any = any || live[t];
        }
        if constexpr (SEL) {
            if (__ballot(any) == 0) continue;
        }
        long long r[SQ_T];
#pragma unroll
        for (int t = 0; t < SQ_T; ++t) r[t] = row[t] < hi ? row[t] : hi - 1;        // stay inside the list; masked below
        float s[SQ_T];
        sq_score_loads<Codec>(codes, d, C, c, r, w, s);
#pragma unroll
        for (int t = 0; t < SQ_T; ++t) {
            const u64 key = make_key(Sense::key_score(Sense::value(base, s[t])), (unsigned)row[t]);
            wl.offer(live[t] && c == 0 && key > wl.tau, key, lane);
        }
    }

    wl.compact(lane);
    __syncthreads();
    if (wave == 0) {
        for (int w = 1; w < 4; ++w) {
            const u64* other = reinterpret_cast<const u64*>(smem) + (size_t)w * cap;
            for (int i0 = 0; i0 < k; i0 += 64) {
                const int i = i0 + lane;
                const u64 key = i < k ? other[i] : 0;
                wl.offer(key != 0 && key > wl.tau, key, lane);
            }
        }
        wl.compact(lane);
        for (int i = lane; i < k; i += 64) dst[i] = wl.buf[i];
    }
}

// grid = nq * nprobe: block b scans the list probes[b] of query b / nprobe; its k keys go to part[(b % nprobe) * nq + b / nprobe]
template <class Codec, bool SEL, class Sense = SenseIP>
__global__ __launch_bounds__(256) void sq_scan_kernel(const unsigned char* __restrict__ codes, const long long* __restrict__ list_off,
                                                      int nlist, const float* __restrict__ W, const float* __restrict__ q0,
                                                      const long long* __restrict__ probes, const float* __restrict__ bias, int nprobe,
                                                      int nq, int d, int k, int cap, u64* __restrict__ part,
                                                      const unsigned* __restrict__ keep) {
    const int qi = blockIdx.x / nprobe, pi = blockIdx.x - qi * nprobe;
    const long long l = probes[(size_t)qi * nprobe + pi];
    long long lo = 0, hi = 0;
    if (l >= 0 && l < nlist) { lo = list_off[l]; hi = list_off[l + 1]; }          // block-uniform
    sq_scan_list<Codec, SEL, Sense>(codes, lo, hi, W + (size_t)qi * d, Sense::template base<Codec>(bias, (size_t)qi * nprobe + pi, q0, qi),
                                    d, k, cap, part + ((size_t)pi * nq + qi) * k, keep);
}

// wise_ivfsq_scan_local.  grid = nq * nprobe: block b is probe group b / nq of query b % nq — group-major, so the blocks that
// have a group are the first ones of the grid and follow each other: workgroups go to the XCDs round-robin by number, and with
// the groups innermost the few live blocks of every query (numbers q * nprobe + 0 .. used - 1) would land on the same few XCDs.
// probes / bias are the compacted ones (compact_probes_bias_kernel with G = nprobe and a share of 1: used[q] = the probes kept =
// the groups of query q, one kept probe each); a block past used[q] returns BEFORE it loads the query's weight row, and its slot
// of part is never read: the merge folds used[q] lists.  list_off is clipped to the slice, rows are positions in the slice.
template <class Codec, class Sense = SenseIP>
__global__ __launch_bounds__(256) void sq_scan_local_kernel(const unsigned char* __restrict__ codes, const long long* __restrict__ list_off,
                                                            int nlist, const float* __restrict__ W, const float* __restrict__ q0,
                                                            const long long* __restrict__ probes, const float* __restrict__ bias,
                                                            int nprobe, int nq, int d, int k, int cap, u64* __restrict__ part,
                                                            const int* __restrict__ used) {
    const int g = blockIdx.x / nq, qi = blockIdx.x - g * nq;
    if (g >= used[qi]) return;                                                      // block-uniform
    const long long l = probes[(size_t)qi * nprobe + g];
    long long lo = 0, hi = 0;
    if (l >= 0 && l < nlist) { lo = list_off[l]; hi = list_off[l + 1]; }
    sq_scan_list<Codec, false, Sense>(codes, lo, hi, W + (size_t)qi * d, Sense::template base<Codec>(bias, (size_t)qi * nprobe + g, q0, qi),
                                      d, k, cap, part + ((size_t)g * nq + qi) * k, nullptr);
}

// ---- range_search (wise_ivfsq_range_*): every row of the probed lists with (bias + q0) + s_0 > radius, s_0 from sq_score_loads
// (SenseL2, wise_ivfl2_range_*: s_0 < radius).
// One block per (query, probe) as sq_scan_kernel; structure, workspace and the determinism argument: range_common.h
template <class Codec>
struct SqLane {
    int C, RPL, sub, c;
    bool active;
    float4 w[4];
    __device__ __forceinline__ void init(const float* __restrict__ wrow, int d, int lane) {
        C = d >> 4; RPL = 64 / C; sub = lane / C; c = lane - sub * C; active = sub < RPL;
        Codec::weights(wrow, d, c, w);
    }
};

template <class Codec, class Sense = SenseIP>
__global__ __launch_bounds__(256) void sq_range_count_kernel(const unsigned char* __restrict__ codes, const long long* __restrict__ list_off,
                                                             int nlist, const float* __restrict__ W, const float* __restrict__ q0,
                                                             const long long* __restrict__ probes, const float* __restrict__ bias,
                                                             int nprobe, int d, float radius, const unsigned* __restrict__ keep,
                                                             unsigned* __restrict__ hit, long long wstride, long long* __restrict__ seg) {
    __shared__ unsigned hb[RANGE_WORDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qi = blockIdx.x / nprobe, pi = blockIdx.x - qi * nprobe;
    const long long l = probes[(size_t)qi * nprobe + pi];
    long long lo = 0, hi = 0;
    if (l >= 0 && l < nlist) { lo = list_off[l]; hi = list_off[l + 1]; }            // block-uniform
    const float base = Sense::template base<Codec>(bias, (size_t)qi * nprobe + pi, q0, qi);
    SqLane<Codec> L;
    L.init(W + (size_t)qi * d, d, lane);
    unsigned* dst = hit + (size_t)qi * wstride + (lo >> 5) + (l > 0 ? l : 0);
    long long total = 0;
    for (long long clo = lo; clo < hi; clo += RANGE_ROWS, dst += RANGE_WORDS) {
        const long long chi = clo + RANGE_ROWS < hi ? clo + RANGE_ROWS : hi;
        if (wave == 0) hb[lane] = 0u;
        __syncthreads();
        const int ngroups = (int)((chi - clo + L.RPL - 1) / L.RPL);
        for (int g = wave * SQ_T; g < ngroups; g += 4 * SQ_T) {                     // wave-uniform
            long long r[SQ_T];
            bool live[SQ_T];
            bool any = false;
#pragma unroll
            for (int t = 0; t < SQ_T; ++t) {
                r[t] = clo + (long long)(g + t) * L.RPL + L.sub;
                live[t] = L.active && r[t] < chi;
                if (keep) live[t] = live[t] && ((keep[r[t] >> 5] >> (r[t] & 31)) & 1u) != 0;
                any = any || live[t];
                if (r[t] >= chi) r[t] = chi - 1;                                    // stay inside the list; masked by live
            }
            if (keep && __ballot(any) == 0) continue;
            float s[SQ_T];
            sq_score_loads<Codec>(codes, d, L.C, L.c, r, L.w, s);
#pragma unroll
            for (int t = 0; t < SQ_T; ++t)
                if (live[t] && L.c == 0 && Sense::range_hit(Sense::value(base, s[t]), radius)) range_mark(hb, (int)(r[t] - clo));
        }
        __syncthreads();
        if (wave == 0) total += range_publish(hb, dst, (int)((chi - clo + 31) >> 5), lane);
    }
    if (threadIdx.x == 0) seg[(size_t)qi * (nprobe + 1) + pi] = total;
}

// ---- search_grouped, stage 1 (group_topk.hip holds stages 2 and 3): sq_range_count_kernel with the hit mark replaced by one store.
// ord[q][r] = f32_order(Sense::key_score(value)) — the upper half of the key sq_scan_list makes of that (query, row) — for every row
// r of the probed lists; a row cleared in keep reads 0, the keys' empty value.  A chunk's images are gathered in LDS and leave as
// one run of 4-byte words.  Probed lists are distinct, so every (query, row) is stored at most once; the rows of the lists a query
// does not probe are not written (the entry point clears ord first).
template <class Codec, class Sense = SenseIP>
__global__ __launch_bounds__(256) void sq_group_scores_kernel(const unsigned char* __restrict__ codes, long long N,
                                                              const long long* __restrict__ list_off, int nlist, const float* __restrict__ W,
                                                              const float* __restrict__ q0, const long long* __restrict__ probes,
                                                              const float* __restrict__ bias, int nprobe, int d,
                                                              const unsigned* __restrict__ keep, unsigned* __restrict__ ord) {
    __shared__ unsigned sc[RANGE_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qi = blockIdx.x / nprobe, pi = blockIdx.x - qi * nprobe;
    const long long l = probes[(size_t)qi * nprobe + pi];
    long long lo = 0, hi = 0;
    if (l >= 0 && l < nlist) { lo = list_off[l]; hi = list_off[l + 1]; }            // block-uniform
    if (lo < 0) lo = 0;
    if (hi > N) hi = N;                                                             // never past ord's row, whatever list_off holds
    const float base = Sense::template base<Codec>(bias, (size_t)qi * nprobe + pi, q0, qi);
    SqLane<Codec> L;
    L.init(W + (size_t)qi * d, d, lane);
    unsigned* dst = ord + (size_t)qi * (size_t)N;
    for (long long clo = lo; clo < hi; clo += RANGE_ROWS) {
        const long long chi = clo + RANGE_ROWS < hi ? clo + RANGE_ROWS : hi;
        for (int i = threadIdx.x; i < RANGE_ROWS; i += 256) sc[i] = 0u;
        __syncthreads();
        const int ngroups = (int)((chi - clo + L.RPL - 1) / L.RPL);
        for (int g = wave * SQ_T; g < ngroups; g += 4 * SQ_T) {                     // wave-uniform
            long long r[SQ_T];
            bool live[SQ_T];
            bool any = false;
#pragma unroll
            for (int t = 0; t < SQ_T; ++t) {
                r[t] = clo + (long long)(g + t) * L.RPL + L.sub;
                live[t] = L.active && r[t] < chi;
                if (r[t] >= chi) r[t] = chi - 1;                                    // stay inside the list; masked by live
                if (keep) live[t] = live[t] && ((keep[r[t] >> 5] >> (r[t] & 31)) & 1u) != 0;
                any = any || live[t];
            }
            if (keep && __ballot(any) == 0) continue;
            float s[SQ_T];
            sq_score_loads<Codec>(codes, d, L.C, L.c, r, L.w, s);
#pragma unroll
            for (int t = 0; t < SQ_T; ++t)
                if (live[t] && L.c == 0) sc[(int)(r[t] - clo)] = f32_order(Sense::key_score(Sense::value(base, s[t])));
        }
        __syncthreads();
        for (int i = threadIdx.x; i < (int)(chi - clo); i += 256) dst[clo + i] = sc[i];
        __syncthreads();
    }
}

template <class Codec, class Sense = SenseIP>
__global__ __launch_bounds__(256) void sq_range_fill_kernel(const unsigned char* __restrict__ codes, const long long* __restrict__ list_off,
                                                            int nlist, const long long* __restrict__ ids, const float* __restrict__ W,
                                                            const float* __restrict__ q0, const long long* __restrict__ probes,
                                                            const float* __restrict__ bias, int nprobe, int d,
                                                            const unsigned* __restrict__ hit, long long wstride,
                                                            const long long* __restrict__ seg, const long long* __restrict__ lims,
                                                            float* __restrict__ outD, long long* __restrict__ outI) {
    __shared__ unsigned short lst[RANGE_ROWS];
    __shared__ int s_cnt;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qi = blockIdx.x / nprobe, pi = blockIdx.x - qi * nprobe;
    const long long* so = seg + (size_t)qi * (nprobe + 1) + pi;
    long long left = so[1] - so[0];                              // hits count found in this segment: never more are written
    if (left <= 0) return;                                                     // no hit in this list (block-uniform)
    long long dest = lims[qi] + so[0];
    const long long l = probes[(size_t)qi * nprobe + pi];
    if (l < 0 || l >= nlist) return;                                                // not the probes count saw: nothing to read
    const long long lo = list_off[l], hi = list_off[l + 1];
    const unsigned* words = hit + (size_t)qi * wstride + (lo >> 5) + l;
    const float base = Sense::template base<Codec>(bias, (size_t)qi * nprobe + pi, q0, qi);
    SqLane<Codec> L;
    L.init(W + (size_t)qi * d, d, lane);
    for (long long clo = lo; clo < hi; clo += RANGE_ROWS, words += RANGE_WORDS) {
        const long long chi = clo + RANGE_ROWS < hi ? clo + RANGE_ROWS : hi;
        if (wave == 0) {
            const int n = range_list(words, (int)((chi - clo + 31) >> 5), lst, lane);
            if (lane == 0) s_cnt = n;
        }
        __syncthreads();
        const int cnt = s_cnt < left ? s_cnt : (int)left;
        const int ngroups = (cnt + L.RPL - 1) / L.RPL;
        for (int g = wave * SQ_T; g < ngroups; g += 4 * SQ_T) {
            long long r[SQ_T];
            int e[SQ_T];
#pragma unroll
            for (int t = 0; t < SQ_T; ++t) {
                e[t] = (g + t) * L.RPL + L.sub;
                if (!L.active || e[t] >= cnt) e[t] = -1;
                r[t] = clo + lst[e[t] >= 0 ? e[t] : cnt - 1];
            }
            float s[SQ_T];
            sq_score_loads<Codec>(codes, d, L.C, L.c, r, L.w, s);
#pragma unroll
            for (int t = 0; t < SQ_T; ++t)
                if (e[t] >= 0 && L.c == 0) {
                    outD[dest + e[t]] = Sense::value(base, s[t]);
                    outI[dest + e[t]] = ids ? ids[r[t]] : r[t];
                }
        }
        __syncthreads();
        dest += cnt;
        left -= cnt;
    }
}

static bool scan_shape_ok(int nq, int nprobe, int k) {
    return nq >= 1 && nq <= 65535 && nprobe >= 1 && nprobe <= 2048 && k >= 1 && k <= 2048;
}

}  // namespace ivf_sq
}  // namespace wise

using namespace wise;
using namespace wise::ivf_sq;

#define SQ_CHECK_SHAPE(what) WISE_CHECK_ARG(sq_shape_ok(d), what ": d=%d unsupported (d %% 16 == 0 in [16, 1024])", d)

extern "C" int wise_sq_train(const float* resid, int64_t n, int d, float* trained, void* stream) {
    SQ_CHECK_SHAPE("sq_train");
    WISE_CHECK_ARG(n >= 1 && resid && trained, "sq_train: bad argument (n >= 1)");
    hipStream_t st = (hipStream_t)stream;
    unsigned* cells = reinterpret_cast<unsigned*>(trained);
    hipLaunchKernelGGL(train_init_kernel, dim3((2 * d + 255) / 256), dim3(256), 0, st, cells, d);
    WISE_LAUNCH_CHECK("sq train_init_kernel");
    long long slabs = (n + 3) / 4;
    if (slabs > 1024) slabs = 1024;
    hipLaunchKernelGGL(train_minmax_kernel, dim3((d + 63) / 64, (unsigned)slabs), dim3(256), 0, st, resid, (long long)n, d, cells, cells + d);
    WISE_LAUNCH_CHECK("sq train_minmax_kernel");
    hipLaunchKernelGGL(train_finish_kernel, dim3((d + 255) / 256), dim3(256), 0, st, trained, d);
    WISE_LAUNCH_CHECK("sq train_finish_kernel");
    return WISE_OK;
}

extern "C" int wise_sq_minmax(const float* rows, int64_t n, int d, float* lo, float* hi, int accumulate, void* stream) {
    SQ_CHECK_SHAPE("sq_minmax");
    WISE_CHECK_ARG(n >= 0 && lo && hi && lo != hi && (rows || n == 0), "sq_minmax: bad argument");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(minmax_open_kernel, dim3((d + 255) / 256), dim3(256), 0, st, lo, hi, d, accumulate);
    WISE_LAUNCH_CHECK("sq minmax_open_kernel");
    if (n > 0) {
        long long slabs = (n + 3) / 4;
        if (slabs > 1024) slabs = 1024;
        hipLaunchKernelGGL(train_minmax_kernel, dim3((d + 63) / 64, (unsigned)slabs), dim3(256), 0, st, rows, (long long)n, d,
                           reinterpret_cast<unsigned*>(lo), reinterpret_cast<unsigned*>(hi));
        WISE_LAUNCH_CHECK("sq train_minmax_kernel");
    }
    hipLaunchKernelGGL(minmax_close_kernel, dim3((d + 255) / 256), dim3(256), 0, st, lo, hi, d);
    WISE_LAUNCH_CHECK("sq minmax_close_kernel");
    return WISE_OK;
}

extern "C" int wise_sq_encode(const float* resid, const float* trained, int64_t n, int d, uint8_t* codes, void* stream) {
    SQ_CHECK_SHAPE("sq_encode");
    WISE_CHECK_ARG(n >= 0 && n < (1ll << 31) && trained && (n == 0 || (resid && codes)), "sq_encode: bad argument");
    if (n == 0) return WISE_OK;
    const long long total = (long long)n * d;
    hipLaunchKernelGGL(encode_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, resid, trained, total, d,
                       codes);
    WISE_LAUNCH_CHECK("sq encode_kernel");
    return WISE_OK;
}

extern "C" int wise_sq_query(const float* Q, const float* trained, int nq, int d, float* W, float* q0, void* stream) {
    SQ_CHECK_SHAPE("sq_query");
    WISE_CHECK_ARG(nq >= 0 && nq <= 65535 && trained && (nq == 0 || (Q && W && q0)), "sq_query: bad argument (nq <= 65535)");
    if (nq == 0) return WISE_OK;
    hipLaunchKernelGGL(query_kernel, dim3(nq), dim3(64), 0, (hipStream_t)stream, Q, trained, d, W, q0);
    WISE_LAUNCH_CHECK("sq query_kernel");
    return WISE_OK;
}

extern "C" int wise_sq_decode(const uint8_t* codes, int64_t N, const int64_t* pos, int rows, const int64_t* list_off, int nlist,
                              const float* centroids, const float* trained, int d, float* out, void* stream) {
    SQ_CHECK_SHAPE("sq_decode");
    WISE_CHECK_ARG(N >= 0 && rows >= 0 && nlist >= 1 && list_off && centroids && trained && (N == 0 || codes) && (rows == 0 || (pos && out)),
                   "sq_decode: bad argument");
    if (rows == 0) return WISE_OK;
    hipLaunchKernelGGL(decode_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, codes, (long long)N, (const long long*)pos,
                       (const long long*)list_off, nlist, centroids, trained, d, out);
    WISE_LAUNCH_CHECK("sq decode_kernel");
    return WISE_OK;
}

extern "C" size_t wise_ivfsq_scan_workspace_bytes(int nq, int nprobe, int k) {
    if (!scan_shape_ok(nq, nprobe, k)) return 0;
    return align_up((size_t)nq * nprobe * k * sizeof(u64), 256);
}

// Workspace of the rank-local scan (LocalWorkspace, probe_compact.h): the keys are [nprobe][nq][k]
extern "C" size_t wise_ivfsq_scan_local_workspace_bytes(int nq, int nprobe, int k) {
    const size_t part = wise_ivfsq_scan_workspace_bytes(nq, nprobe, k);
    if (part == 0) return 0;
    return LocalWorkspace::bytes(part, nq, nprobe);
}

// wise_ivfsq_scan / wise_ivfsq16_scan and, with keep, their _sel forms.  Codec16 has no q0
template <class Codec, class Sense = SenseIP>
static int sq_scan_impl(const char* what, const void* codes, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                        const float* W, const float* q0, int nq, const int64_t* probes, const float* bias, int nprobe, int k, float* outD,
                        int64_t* outI, void* workspace, size_t workspace_bytes, void* stream, const uint32_t* keep) {
    constexpr bool HAS_Q0 = Codec::PIECES == 1;
    constexpr const char* ALIGNED = Sense::FLIP ? "X and Q" : "codes and W";
    WISE_CHECK_ARG(sq_shape_ok(d), "%s: d=%d unsupported (d %% 16 == 0 in [16, 1024])", what, d);
    WISE_CHECK_ARG(scan_shape_ok(nq, nprobe, k), "%s: nq=%d nprobe=%d k=%d unsupported (nq <= 65535, nprobe <= 2048, k <= 2048)", what, nq,
                   nprobe, k);
    WISE_CHECK_ARG(nlist >= 1 && N >= 0 && N < 0xFFFFFFFFll, "%s: N=%lld nlist=%d out of range", what, (long long)N, nlist);
    WISE_CHECK_ARG(W && (q0 || !HAS_Q0) && probes && (bias || Sense::FLIP) && outD && outI && list_off && (codes || N == 0),
                   "%s: null pointer", what);
    WISE_CHECK_ARG(((uintptr_t)codes & 15) == 0 && ((uintptr_t)W & 15) == 0, "%s: %s must be 16-byte aligned", what, ALIGNED);
    const size_t need = wise_ivfsq_scan_workspace_bytes(nq, nprobe, k);
    WISE_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace %zu < %zu bytes", what, workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    u64* part = reinterpret_cast<u64*>(workspace);
    const int cap = topk_list_cap(k);
    const size_t lds = (size_t)4 * cap * 8;
    auto kern = keep ? sq_scan_kernel<Codec, true, Sense> : sq_scan_kernel<Codec, false, Sense>;
    if (lds > 48 * 1024) raise_lds_limit(reinterpret_cast<const void*>(kern), (int)lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)((long long)nq * nprobe)), dim3(256), lds, st, reinterpret_cast<const unsigned char*>(codes),
                       (const long long*)list_off, nlist, W, q0, (const long long*)probes, bias, nprobe, nq, d, k, cap, part, keep);
    WISE_LAUNCH_CHECK("sq_scan_kernel");
    if (int rc = merge_lists_launch(part, nprobe, nq, k, reinterpret_cast<const long long*>(ids), outD, reinterpret_cast<long long*>(outI), st))
        return rc;
    if constexpr (Sense::FLIP) return l2_flip_launch(outD, nq * k, nullptr, st);     // scores and padding become distances again
    return WISE_OK;
}

extern "C" int wise_ivfsq_scan(const uint8_t* codes, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                               const float* W, const float* q0, int nq, const int64_t* probes, const float* bias, int nprobe, int k,
                               float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream) {
    return sq_scan_impl<Codec8>("ivfsq_scan", codes, N, d, list_off, nlist, ids, W, q0, nq, probes, bias, nprobe, k, outD, outI, workspace,
                                workspace_bytes, stream, nullptr);
}

extern "C" int wise_ivfsq_scan_sel(const uint8_t* codes, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                                   const float* W, const float* q0, int nq, const int64_t* probes, const float* bias, int nprobe, int k,
                                   const uint32_t* keep, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    WISE_CHECK_ARG(keep || N == 0, "ivfsq_scan_sel: null bitmap");
    return sq_scan_impl<Codec8>("ivfsq_scan_sel", codes, N, d, list_off, nlist, ids, W, q0, nq, probes, bias, nprobe, k, outD, outI,
                                workspace, workspace_bytes, stream, keep);
}

extern "C" int wise_ivfsq16_scan(const uint16_t* halves, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                                 const float* Q, int nq, const int64_t* probes, const float* bias, int nprobe, int k, float* outD,
                                 int64_t* outI, void* workspace, size_t workspace_bytes, void* stream) {
    return sq_scan_impl<Codec16>("ivfsq16_scan", halves, N, d, list_off, nlist, ids, Q, nullptr, nq, probes, bias, nprobe, k, outD, outI,
                                 workspace, workspace_bytes, stream, nullptr);
}

extern "C" int wise_ivfsq16_scan_sel(const uint16_t* halves, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                                     const float* Q, int nq, const int64_t* probes, const float* bias, int nprobe, int k,
                                     const uint32_t* keep, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    WISE_CHECK_ARG(keep || N == 0, "ivfsq16_scan_sel: null bitmap");
    return sq_scan_impl<Codec16>("ivfsq16_scan_sel", halves, N, d, list_off, nlist, ids, Q, nullptr, nq, probes, bias, nprobe, k, outD,
                                 outI, workspace, workspace_bytes, stream, keep);
}

template <class Codec, class Sense = SenseIP>
static int sq_scan_local_impl(const char* what, const void* codes, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                              const float* W, const float* q0, int nq, const int64_t* probes, const float* bias, int nprobe, int k,
                              int64_t pos_base, float* outD, int64_t* outI, int32_t* probe_count, void* workspace, size_t workspace_bytes,
                              void* stream) {
    constexpr bool HAS_Q0 = Codec::PIECES == 1;
    constexpr const char* ALIGNED = Sense::FLIP ? "X and Q" : "codes and W";
    WISE_CHECK_ARG(sq_shape_ok(d), "%s: d=%d unsupported (d %% 16 == 0 in [16, 1024])", what, d);
    WISE_CHECK_ARG(scan_shape_ok(nq, nprobe, k), "%s: nq=%d nprobe=%d k=%d unsupported (nq <= 65535, nprobe <= 2048, k <= 2048)", what, nq,
                   nprobe, k);
    WISE_CHECK_ARG(nlist >= 1 && N >= 0 && N < 0xFFFFFFFFll && pos_base >= 0, "%s: N=%lld nlist=%d pos_base=%lld out of range", what,
                   (long long)N, nlist, (long long)pos_base);
    WISE_CHECK_ARG(W && (q0 || !HAS_Q0) && probes && (bias || Sense::FLIP) && outD && outI && list_off && (codes || N == 0),
                   "%s: null pointer", what);
    WISE_CHECK_ARG(((uintptr_t)codes & 15) == 0 && ((uintptr_t)W & 15) == 0, "%s: %s must be 16-byte aligned", what, ALIGNED);
    const size_t need = wise_ivfsq_scan_local_workspace_bytes(nq, nprobe, k);
    WISE_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace %zu < %zu bytes", what, workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const LocalWorkspace lw = LocalWorkspace::carve(workspace, wise_ivfsq_scan_workspace_bytes(nq, nprobe, k), nq, nprobe, probe_count);
    const long long* lo = reinterpret_cast<const long long*>(list_off);
    hipLaunchKernelGGL(compact_probes_bias_kernel<!Sense::FLIP>, dim3(nq), dim3(64), 0, st, reinterpret_cast<const long long*>(probes), bias,
                       nprobe, lo, nlist, nprobe, 1, lw.live, lw.lbias, lw.count, lw.used);
    WISE_LAUNCH_CHECK("compact_probes_bias_kernel");
    const int cap = topk_list_cap(k);
    const size_t lds = (size_t)4 * cap * 8;
    if (lds > 48 * 1024) raise_lds_limit(reinterpret_cast<const void*>(sq_scan_local_kernel<Codec, Sense>), (int)lds);
    hipLaunchKernelGGL((sq_scan_local_kernel<Codec, Sense>), dim3((unsigned)((long long)nq * nprobe)), dim3(256), lds, st,
                       reinterpret_cast<const unsigned char*>(codes), lo, nlist, W, q0, lw.live, lw.lbias, nprobe, nq, d, k, cap, lw.part,
                       lw.used);
    WISE_LAUNCH_CHECK("sq_scan_local_kernel");
    // keys carry local rows; without ids the merge writes pos_base + row, the row's position in the whole array
    if (int rc = merge_lists_launch(lw.part, nprobe, nq, k, reinterpret_cast<const long long*>(ids), outD, reinterpret_cast<long long*>(outI),
                                    st, lw.used, (long long)pos_base))
        return rc;
    if constexpr (Sense::FLIP) return l2_flip_launch(outD, nq * k, nullptr, st);
    return WISE_OK;
}

extern "C" int wise_ivfsq_scan_local(const uint8_t* codes, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                                     const float* W, const float* q0, int nq, const int64_t* probes, const float* bias, int nprobe,
                                     int k, int64_t pos_base, float* outD, int64_t* outI, int32_t* probe_count, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    return sq_scan_local_impl<Codec8>("ivfsq_scan_local", codes, N, d, list_off, nlist, ids, W, q0, nq, probes, bias, nprobe, k, pos_base,
                                      outD, outI, probe_count, workspace, workspace_bytes, stream);
}

extern "C" int wise_ivfsq16_scan_local(const uint16_t* halves, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                                       const float* Q, int nq, const int64_t* probes, const float* bias, int nprobe, int k,
                                       int64_t pos_base, float* outD, int64_t* outI, int32_t* probe_count, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    return sq_scan_local_impl<Codec16>("ivfsq16_scan_local", halves, N, d, list_off, nlist, ids, Q, nullptr, nq, probes, bias, nprobe, k,
                                       pos_base, outD, outI, probe_count, workspace, workspace_bytes, stream);
}

static bool sq_range_shape_ok(int64_t N, int nlist, int nq, int nprobe) {
    return N >= 0 && N < 0xFFFFFFFFll && nlist >= 1 && nq >= 1 && nq <= 65535 && nprobe >= 1 && nprobe <= 2048;
}

extern "C" size_t wise_ivfsq_range_workspace_bytes(int64_t N, int nlist, int nq, int nprobe) {
    if (!sq_range_shape_ok(N, nlist, nq, nprobe)) return 0;
    return range_workspace_bytes(nq, range_ivf_wstride(N, nlist), nprobe);
}

static int sq_range_args(const char* what, bool has_q0, bool l2, const void* codes, int64_t N, int d, const int64_t* list_off, int nlist,
                         const float* W, const float* q0, int nq, const int64_t* probes, const float* bias, int nprobe, float radius,
                         void* workspace, size_t workspace_bytes) {
    WISE_CHECK_ARG(sq_shape_ok(d), "%s: d=%d unsupported (d %% 16 == 0 in [16, 1024])", what, d);
    WISE_CHECK_ARG(sq_range_shape_ok(N, nlist, nq, nprobe), "%s: N=%lld nlist=%d nq=%d nprobe=%d unsupported (nq <= 65535, nprobe <= 2048)",
                   what, (long long)N, nlist, nq, nprobe);
    WISE_CHECK_ARG(W && (q0 || !has_q0) && probes && (bias || l2) && list_off && (codes || N == 0), "%s: null pointer", what);
    WISE_CHECK_ARG(((uintptr_t)codes & 15) == 0 && ((uintptr_t)W & 15) == 0, "%s: %s must be 16-byte aligned", what,
                   l2 ? "X and Q" : "codes and W");
    WISE_CHECK_ARG(radius == radius && radius - radius == 0.f, "%s: radius must be finite", what);
    const size_t need = wise_ivfsq_range_workspace_bytes(N, nlist, nq, nprobe);
    WISE_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace %zu < %zu bytes", what, workspace_bytes, need);
    return WISE_OK;
}

template <class Codec, class Sense = SenseIP>
static int sq_range_count_impl(const char* what, const void* codes, int64_t N, int d, const int64_t* list_off, int nlist, const float* W,
                               const float* q0, int nq, const int64_t* probes, const float* bias, int nprobe, float radius,
                               const uint32_t* keep, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = sq_range_args(what, Codec::PIECES == 1, Sense::FLIP, codes, N, d, list_off, nlist, W, q0, nq, probes, bias, nprobe, radius,
                               workspace, workspace_bytes))
        return rc;
    WISE_CHECK_ARG(counts, "%s: null pointer", what);
    hipStream_t st = (hipStream_t)stream;
    const long long wstride = range_ivf_wstride(N, nlist);
    unsigned* hit = reinterpret_cast<unsigned*>(workspace);
    long long* seg = reinterpret_cast<long long*>(reinterpret_cast<unsigned char*>(workspace) + range_hit_bytes(nq, wstride));
    hipLaunchKernelGGL((sq_range_count_kernel<Codec, Sense>), dim3((unsigned)((long long)nq * nprobe)), dim3(256), 0, st,
                       reinterpret_cast<const unsigned char*>(codes), (const long long*)list_off, nlist, W, q0, (const long long*)probes, bias,
                       nprobe, d, radius, keep, hit, wstride, seg);
    WISE_LAUNCH_CHECK("sq_range_count_kernel");
    hipLaunchKernelGGL(range_scan_kernel, dim3(nq), dim3(1024), 0, st, seg, (long long)nprobe, reinterpret_cast<long long*>(counts));
    WISE_LAUNCH_CHECK("range_scan_kernel");
    return WISE_OK;
}

template <class Codec, class Sense = SenseIP>
static int sq_range_fill_impl(const char* what, const void* codes, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                              const float* W, const float* q0, int nq, const int64_t* probes, const float* bias, int nprobe, float radius,
                              const int64_t* lims, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = sq_range_args(what, Codec::PIECES == 1, Sense::FLIP, codes, N, d, list_off, nlist, W, q0, nq, probes, bias, nprobe, radius,
                               workspace, workspace_bytes))
        return rc;
    WISE_CHECK_ARG(lims && outD && outI, "%s: null pointer", what);
    const long long wstride = range_ivf_wstride(N, nlist);
    const unsigned* hit = reinterpret_cast<const unsigned*>(workspace);
    const long long* seg = reinterpret_cast<const long long*>(reinterpret_cast<unsigned char*>(workspace) + range_hit_bytes(nq, wstride));
    hipLaunchKernelGGL((sq_range_fill_kernel<Codec, Sense>), dim3((unsigned)((long long)nq * nprobe)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned char*>(codes), (const long long*)list_off, nlist, reinterpret_cast<const long long*>(ids),
                       W, q0, (const long long*)probes, bias, nprobe, d, hit, wstride, seg, reinterpret_cast<const long long*>(lims), outD,
                       reinterpret_cast<long long*>(outI));
    WISE_LAUNCH_CHECK("sq_range_fill_kernel");
    return WISE_OK;
}

extern "C" int wise_ivfsq_range_count(const uint8_t* codes, int64_t N, int d, const int64_t* list_off, int nlist, const float* W,
                                      const float* q0, int nq, const int64_t* probes, const float* bias, int nprobe, float radius,
                                      const uint32_t* keep, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    return sq_range_count_impl<Codec8>("ivfsq_range_count", codes, N, d, list_off, nlist, W, q0, nq, probes, bias, nprobe, radius, keep,
                                       counts, workspace, workspace_bytes, stream);
}

extern "C" int wise_ivfsq_range_fill(const uint8_t* codes, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                                     const float* W, const float* q0, int nq, const int64_t* probes, const float* bias, int nprobe,
                                     float radius, const int64_t* lims, float* outD, int64_t* outI, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    return sq_range_fill_impl<Codec8>("ivfsq_range_fill", codes, N, d, list_off, nlist, ids, W, q0, nq, probes, bias, nprobe, radius, lims,
                                      outD, outI, workspace, workspace_bytes, stream);
}

extern "C" int wise_ivfsq16_range_count(const uint16_t* halves, int64_t N, int d, const int64_t* list_off, int nlist, const float* Q, int nq,
                                        const int64_t* probes, const float* bias, int nprobe, float radius, const uint32_t* keep,
                                        int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    return sq_range_count_impl<Codec16>("ivfsq16_range_count", halves, N, d, list_off, nlist, Q, nullptr, nq, probes, bias, nprobe, radius,
                                        keep, counts, workspace, workspace_bytes, stream);
}

extern "C" int wise_ivfsq16_range_fill(const uint16_t* halves, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                                       const float* Q, int nq, const int64_t* probes, const float* bias, int nprobe, float radius,
                                       const int64_t* lims, float* outD, int64_t* outI, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    return sq_range_fill_impl<Codec16>("ivfsq16_range_fill", halves, N, d, list_off, nlist, ids, Q, nullptr, nq, probes, bias, nprobe,
                                       radius, lims, outD, outI, workspace, workspace_bytes, stream);
}

// search_grouped, stage 1 over the probed lists: ord [nq][N] is cleared, then every candidate (query, row) receives its ordered key score
template <class Codec, class Sense = SenseIP>
static int sq_group_scores_impl(const char* what, const void* codes, int64_t N, int d, const int64_t* list_off, int nlist, const float* W,
                                const float* q0, int nq, const int64_t* probes, const float* bias, int nprobe, const uint32_t* keep,
                                uint32_t* ord, void* stream) {
    constexpr bool has_q0 = Codec::PIECES == 1, l2 = Sense::FLIP;
    WISE_CHECK_ARG(sq_shape_ok(d), "%s: d=%d unsupported (d %% 16 == 0 in [16, 1024])", what, d);
    WISE_CHECK_ARG(sq_range_shape_ok(N, nlist, nq, nprobe), "%s: N=%lld nlist=%d nq=%d nprobe=%d unsupported (nq <= 65535, nprobe <= 2048)",
                   what, (long long)N, nlist, nq, nprobe);
    WISE_CHECK_ARG(W && (q0 || !has_q0) && probes && (bias || l2) && list_off && (codes || N == 0) && (ord || N == 0), "%s: null pointer", what);
    WISE_CHECK_ARG(((uintptr_t)codes & 15) == 0 && ((uintptr_t)W & 15) == 0, "%s: %s must be 16-byte aligned", what,
                   l2 ? "X and Q" : "codes and W");
    if (N == 0) return WISE_OK;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(ord, 0, (size_t)nq * (size_t)N * sizeof(uint32_t), st);
    if (e != hipSuccess) { set_error("%s: memset: %s", what, hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL((sq_group_scores_kernel<Codec, Sense>), dim3((unsigned)((long long)nq * nprobe)), dim3(256), 0, st,
                       reinterpret_cast<const unsigned char*>(codes), (long long)N, (const long long*)list_off, nlist, W, q0,
                       (const long long*)probes, bias, nprobe, d, keep, ord);
    WISE_LAUNCH_CHECK("sq_group_scores_kernel");
    return WISE_OK;
}

extern "C" int wise_ivfsq_group_scores(const uint8_t* codes, int64_t N, int d, const int64_t* list_off, int nlist, const float* W,
                                       const float* q0, int nq, const int64_t* probes, const float* bias, int nprobe, const uint32_t* keep,
                                       uint32_t* ord, void* stream) {
    return sq_group_scores_impl<Codec8>("ivfsq_group_scores", codes, N, d, list_off, nlist, W, q0, nq, probes, bias, nprobe, keep, ord, stream);
}

extern "C" int wise_ivfsq16_group_scores(const uint16_t* halves, int64_t N, int d, const int64_t* list_off, int nlist, const float* Q, int nq,
                                         const int64_t* probes, const float* bias, int nprobe, const uint32_t* keep, uint32_t* ord,
                                         void* stream) {
    return sq_group_scores_impl<Codec16>("ivfsq16_group_scores", halves, N, d, list_off, nlist, Q, nullptr, nq, probes, bias, nprobe, keep, ord,
                                         stream);
}

extern "C" int wise_sq16_encode(const float* resid, int64_t n, int d, uint16_t* halves, void* stream) {
    SQ_CHECK_SHAPE("sq16_encode");
    WISE_CHECK_ARG(n >= 0 && n < (1ll << 31) && (n == 0 || (resid && halves)), "sq16_encode: bad argument");
    if (n == 0) return WISE_OK;
    const long long total = (long long)n * d;
    hipLaunchKernelGGL(encode16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, resid, total,
                       reinterpret_cast<_Float16*>(halves));
    WISE_LAUNCH_CHECK("sq encode16_kernel");
    return WISE_OK;
}

extern "C" int wise_sq16_decode(const uint16_t* halves, int64_t N, const int64_t* pos, int rows, const int64_t* list_off, int nlist,
                                const float* centroids, int d, float* out, void* stream) {
    SQ_CHECK_SHAPE("sq16_decode");
    WISE_CHECK_ARG(N >= 0 && rows >= 0 && nlist >= 1 && list_off && centroids && (N == 0 || halves) && (rows == 0 || (pos && out)),
                   "sq16_decode: bad argument");
    if (rows == 0) return WISE_OK;
    hipLaunchKernelGGL(decode16_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const _Float16*>(halves),
                       (long long)N, (const long long*)pos, (const long long*)list_off, nlist, centroids, d, out);
    WISE_LAUNCH_CHECK("sq decode16_kernel");
    return WISE_OK;
}

// ---- IndexIVFFlatL2: the same bodies over CodecL2 (raw fp32 rows, the query itself as the weight row, no bias, no q0) under SenseL2.
// A row's distance is wise_l2_topk_f32's, bit for bit: both are s_0 of sq_score_loads<CodecL2>.
extern "C" size_t wise_ivfl2_scan_workspace_bytes(int nq, int nprobe, int k) { return wise_ivfsq_scan_workspace_bytes(nq, nprobe, k); }

extern "C" size_t wise_ivfl2_scan_local_workspace_bytes(int nq, int nprobe, int k) {
    return wise_ivfsq_scan_local_workspace_bytes(nq, nprobe, k);
}

extern "C" int wise_ivfl2_scan(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids, const float* Q,
                               int nq, const int64_t* probes, int nprobe, int k, float* outD, int64_t* outI, void* workspace,
                               size_t workspace_bytes, void* stream) {
    return sq_scan_impl<CodecL2, SenseL2>("ivfl2_scan", X, N, d, list_off, nlist, ids, Q, nullptr, nq, probes, nullptr, nprobe, k, outD, outI,
                                          workspace, workspace_bytes, stream, nullptr);
}

extern "C" int wise_ivfl2_scan_sel(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids, const float* Q,
                                   int nq, const int64_t* probes, int nprobe, int k, const uint32_t* keep, float* outD, int64_t* outI,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    WISE_CHECK_ARG(keep || N == 0, "ivfl2_scan_sel: null bitmap");
    return sq_scan_impl<CodecL2, SenseL2>("ivfl2_scan_sel", X, N, d, list_off, nlist, ids, Q, nullptr, nq, probes, nullptr, nprobe, k, outD,
                                          outI, workspace, workspace_bytes, stream, keep);
}

extern "C" int wise_ivfl2_scan_local(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                                     const float* Q, int nq, const int64_t* probes, int nprobe, int k, int64_t pos_base, float* outD,
                                     int64_t* outI, int32_t* probe_count, void* workspace, size_t workspace_bytes, void* stream) {
    return sq_scan_local_impl<CodecL2, SenseL2>("ivfl2_scan_local", X, N, d, list_off, nlist, ids, Q, nullptr, nq, probes, nullptr, nprobe, k,
                                                pos_base, outD, outI, probe_count, workspace, workspace_bytes, stream);
}

extern "C" size_t wise_ivfl2_range_workspace_bytes(int64_t N, int nlist, int nq, int nprobe) {
    return wise_ivfsq_range_workspace_bytes(N, nlist, nq, nprobe);
}

extern "C" int wise_ivfl2_range_count(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const float* Q, int nq,
                                      const int64_t* probes, int nprobe, float radius, const uint32_t* keep, int64_t* counts,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    return sq_range_count_impl<CodecL2, SenseL2>("ivfl2_range_count", X, N, d, list_off, nlist, Q, nullptr, nq, probes, nullptr, nprobe,
                                                 radius, keep, counts, workspace, workspace_bytes, stream);
}

extern "C" int wise_ivfl2_range_fill(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const int64_t* ids,
                                     const float* Q, int nq, const int64_t* probes, int nprobe, float radius, const int64_t* lims,
                                     float* outD, int64_t* outI, void* workspace, size_t workspace_bytes, void* stream) {
    return sq_range_fill_impl<CodecL2, SenseL2>("ivfl2_range_fill", X, N, d, list_off, nlist, ids, Q, nullptr, nq, probes, nullptr, nprobe,
                                                radius, lims, outD, outI, workspace, workspace_bytes, stream);
}

extern "C" int wise_ivfl2_group_scores(const float* X, int64_t N, int d, const int64_t* list_off, int nlist, const float* Q, int nq,
                                       const int64_t* probes, int nprobe, const uint32_t* keep, uint32_t* ord, void* stream) {
    return sq_group_scores_impl<CodecL2, SenseL2>("ivfl2_group_scores", X, N, d, list_off, nlist, Q, nullptr, nq, probes, nullptr, nprobe, keep,
                                                  ord, stream);
}

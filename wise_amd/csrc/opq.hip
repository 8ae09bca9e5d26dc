// IndexIVFOPQ — a learned orthonormal rotation R [d,d] in front of the product quantizer (faiss OPQMatrix + IndexIVFPQ).  With
// r = x - c_l and R orthonormal, q . x = q . c_l + (R q) . (R r): rows are encoded from R r, the per-query table is built from R q,
// and everything else of the IndexIVFPQ search (bias, scan, re-ranking) is untouched (ivf_pq.hip, ivf_refine.hip).
//   wise_opq_rotate   out[i, a] = sum_b x[i, b] R[a, b]: one index-ordered fmaf chain over b per output, on the VALU (a matrix-core
//                     product would add in its own order).  A workgroup keeps a tile of 32 rows in LDS, read from memory once,
//                     and walks R in tiles of 64 outputs x 32 inputs staged through LDS; each thread owns 2 rows x 4 outputs.
//                     Few rows (queries): the outputs are split over grid.y so that one query still fills d / 64 workgroups.
//   wise_opq_corr     M[a, b] = sum_i cw_i[a] x[i, b] in fp64, cw_i = the codewords of row i looked up from its m code bytes:
//                     the matrix whose SVD gives the next rotation of the trainer.  Rows ascending inside blocks of 4096 rows,
//                     the blocks' partial matrices added in ascending order.
//   wise_opq_decode   reconstruct_batch: c_l + R^T cw
#include "common.h"

namespace wise {
namespace opq {

constexpr int KSUB = 256;
constexpr int ROT_ROWS = 32;              // rows per workgroup of the rotation
constexpr int ROT_TA = 64;                // outputs per tile of R
constexpr int ROT_KB = 32;                // inputs per tile of R
constexpr int ROT_RSTRIDE = ROT_KB + 4;   // floats per staged row of R: rows a, a+1, ... start 36 floats apart, so the 16 float4
                                          // reads of a quarter wave (rows tx) fall on 16 disjoint groups of 4 banks
constexpr int ROT_PAD = 4;                // floats added to a staged row of x (rows 2 ty land 8 banks apart when d % 64 == 0)
constexpr int MAX_D = 1024;
constexpr int CORR_ROWS = 4096;           // rows per partial matrix of the correlation: part of the contract (the order of the sum)
constexpr int CORR_T = 64;                // a workgroup owns a 64 x 64 tile of M
constexpr int CORR_CHUNK = 16;            // rows staged per step

// grid (row tiles, splits): the workgroup rotates rows [32 bx, 32 bx + 32) for the output tiles ta = by, by + splits, ...
// thread t: ty = t / 16 -> rows 2 ty, 2 ty + 1;  tx = t % 16 -> outputs a0 + tx + 16 j, j = 0 .. 3
__global__ __launch_bounds__(256) void rotate_kernel(const float* __restrict__ x, const float* __restrict__ R, long long n, int d,
                                                     float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int xstride = d + ROT_PAD;
    float* xs = reinterpret_cast<float*>(smem);                       // [ROT_ROWS][d + 4]
    float* rs = xs + (size_t)ROT_ROWS * xstride;                      // [ROT_TA][ROT_RSTRIDE]
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const long long row0 = (long long)blockIdx.x * ROT_ROWS;
    const int d4 = d >> 2;
    for (int i = t; i < ROT_ROWS * d4; i += 256) {
        const int r = i / d4, c = i - r * d4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + r < n) v = *reinterpret_cast<const float4*>(x + (size_t)(row0 + r) * d + 4 * c);
        *reinterpret_cast<float4*>(xs + (size_t)r * xstride + 4 * c) = v;
    }
    const float* x0 = xs + (size_t)(2 * ty) * xstride;
    const float* x1 = x0 + xstride;
    const int tiles = (d + ROT_TA - 1) / ROT_TA;
    for (int ta = blockIdx.y; ta < tiles; ta += gridDim.y) {
        const int a0 = ta * ROT_TA;
        float acc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        for (int b0 = 0; b0 < d; b0 += ROT_KB) {
            const int kb = d - b0 < ROT_KB ? d - b0 : ROT_KB;          // a multiple of 4
            __syncthreads();                                            // the tile of R read in the last step (and xs, first step)
            for (int i = t; i < ROT_TA * (ROT_KB / 4); i += 256) {
                const int al = i >> 3, b4 = (i & 7) * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (a0 + al < d && b4 < kb) v = *reinterpret_cast<const float4*>(R + (size_t)(a0 + al) * d + b0 + b4);
                *reinterpret_cast<float4*>(rs + al * ROT_RSTRIDE + b4) = v;
            }
            __syncthreads();
            for (int b = 0; b < kb; b += 4) {                           // b ascending: the contract's order
                const float4 u0 = *reinterpret_cast<const float4*>(x0 + b0 + b);
                const float4 u1 = *reinterpret_cast<const float4*>(x1 + b0 + b);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float4 w = *reinterpret_cast<const float4*>(rs + (tx + 16 * j) * ROT_RSTRIDE + b);
                    acc[0][j] = fmaf(u0.x, w.x, acc[0][j]);
                    acc[1][j] = fmaf(u1.x, w.x, acc[1][j]);
                    acc[0][j] = fmaf(u0.y, w.y, acc[0][j]);
                    acc[1][j] = fmaf(u1.y, w.y, acc[1][j]);
                    acc[0][j] = fmaf(u0.z, w.z, acc[0][j]);
                    acc[1][j] = fmaf(u1.z, w.z, acc[1][j]);
                    acc[0][j] = fmaf(u0.w, w.w, acc[0][j]);
                    acc[1][j] = fmaf(u1.w, w.w, acc[1][j]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const long long row = row0 + 2 * ty + r;
            if (row >= n) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int a = a0 + tx + 16 * j;
                if (a < d) out[(size_t)row * d + a] = acc[r][j];
            }
        }
    }
}

// grid (b tiles, a tiles, row blocks): P[blk][a][b] = sum over the rows of block blk, ascending, of cw_i[a] * x[i][b] in fp64
// thread t: ty = t / 16 -> a = a0 + ty + 16 i;  tx = t % 16 -> b = b0 + tx + 16 j
__global__ __launch_bounds__(256) void corr_kernel(const unsigned char* __restrict__ codes, const float* __restrict__ cbs,
                                                   const float* __restrict__ x, long long n, int d, int m, double* __restrict__ P) {
    __shared__ float cws[CORR_CHUNK][CORR_T];
    __shared__ float xs[CORR_CHUNK][CORR_T];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int b0 = blockIdx.x * CORR_T, a0 = blockIdx.y * CORR_T, dsub = d / m;
    const long long r0 = (long long)blockIdx.z * CORR_ROWS;
    const long long r1 = r0 + CORR_ROWS < n ? r0 + CORR_ROWS : n;
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    for (long long c0 = r0; c0 < r1; c0 += CORR_CHUNK) {
        __syncthreads();
        for (int e = t; e < CORR_CHUNK * CORR_T; e += 256) {
            const int r = e >> 6, c = e & 63;
            const long long row = c0 + r;
            float cw = 0.f, xv = 0.f;
            if (row < r1) {
                if (a0 + c < d) {
                    const int j = (a0 + c) / dsub, s = (a0 + c) - j * dsub;
                    cw = cbs[((size_t)j * KSUB + codes[(size_t)row * m + j]) * dsub + s];
                }
                if (b0 + c < d) xv = x[(size_t)row * d + b0 + c];
            }
            cws[r][c] = cw;
            xs[r][c] = xv;
        }
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < CORR_CHUNK; ++r) {                          // rows ascending; rows past the block add +0 * +0
            double u[4], v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                u[i] = (double)cws[r][ty + 16 * i];
                v[i] = (double)xs[r][tx + 16 * i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fma(u[i], v[j], acc[i][j]);
        }
    }
    double* dst = P + (size_t)blockIdx.z * d * d;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int a = a0 + ty + 16 * i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = b0 + tx + 16 * j;
            if (a < d && b < d) dst[(size_t)a * d + b] = acc[i][j];
        }
    }
}

// M[e] = P[0][e] + P[1][e] + ... in that order
__global__ __launch_bounds__(256) void corr_fold_kernel(const double* __restrict__ P, int parts, long long dd, double* __restrict__ M) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= dd) return;
    double s = P[e];
    for (int p = 1; p < parts; ++p) s += P[(size_t)p * dd + e];
    M[e] = s;
}

// one workgroup per row: out[c] = c_l[c] + sum_a R[a][c] cw[a], the sum an index-ordered fmaf chain over a from 0
__global__ __launch_bounds__(256) void decode_kernel(const unsigned char* __restrict__ codes, long long N, const long long* __restrict__ pos,
                                                     const long long* __restrict__ list_off, int nlist, const float* __restrict__ cent,
                                                     const float* __restrict__ cbs, const float* __restrict__ R, int d, int m,
                                                     float* __restrict__ out) {
    __shared__ float cw[MAX_D];
    const int dsub = d / m;
    const long long p = pos[blockIdx.x];
    float* o = out + (size_t)blockIdx.x * d;
    if (p < 0 || p >= N) {                                              // block-uniform
        for (int c = threadIdx.x; c < d; c += blockDim.x) o[c] = __builtin_nanf("");
        return;
    }
    int lo = 0, hi = nlist;                       // the last list whose offset is <= p (empty lists share offsets: skip them)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (list_off[mid] <= p) lo = mid; else hi = mid;
    }
    const unsigned char* code = codes + (size_t)p * m;
    for (int a = threadIdx.x; a < d; a += blockDim.x) {
        const int j = a / dsub, s = a - j * dsub;
        cw[a] = cbs[((size_t)j * KSUB + code[j]) * dsub + s];
    }
    __syncthreads();
    const float* cr = cent + (size_t)lo * d;
    for (int c = threadIdx.x; c < d; c += blockDim.x) {
        float acc = 0.f;
        for (int a = 0; a < d; ++a) acc = fmaf(R[(size_t)a * d + c], cw[a], acc);
        o[c] = cr[c] + acc;
    }
}

static bool rot_shape_ok(int d) { return d >= 4 && d <= MAX_D && d % 4 == 0; }
static bool pq_shape_ok(int d, int m) {
    if (d < 2 || m < 1 || m > 128 || d % m) return false;
    const int dsub = d / m;
    return dsub >= 2 && dsub <= 96 && dsub % 2 == 0;
}
static int corr_parts(long long n) { return n <= 0 ? 1 : (int)((n + CORR_ROWS - 1) / CORR_ROWS); }

}  // namespace opq
}  // namespace wise

using namespace wise;
using namespace wise::opq;

extern "C" int wise_opq_rotate(const float* x, const float* R, int64_t n, int d, float* out, void* stream) {
    if (!rot_shape_ok(d)) {
        set_error("opq_rotate: d=%d unsupported (d %% 4 == 0, 4 <= d <= 1024)", d);
        return WISE_E_UNSUPPORTED;
    }
    WISE_CHECK_ARG(n >= 0 && n < (1ll << 31) * ROT_ROWS && R && (n == 0 || (x && out)), "opq_rotate: bad argument");
    WISE_CHECK_ARG(n == 0 || x != out, "opq_rotate: out must not alias x");
    WISE_CHECK_ARG((((uintptr_t)x | (uintptr_t)R | (uintptr_t)out) & 15) == 0, "opq_rotate: x, R and out must be 16-byte aligned");
    if (n == 0) return WISE_OK;
    const long long row_tiles = (n + ROT_ROWS - 1) / ROT_ROWS;
    const int tiles = (d + ROT_TA - 1) / ROT_TA;
    long long splits = (512 + row_tiles - 1) / row_tiles;       // about two workgroups per CU before the rows alone fill the device
    if (splits > tiles) splits = tiles;
    const size_t lds = ((size_t)ROT_ROWS * (d + ROT_PAD) + (size_t)ROT_TA * ROT_RSTRIDE) * 4;
    if (lds > 48 * 1024) raise_lds_limit(reinterpret_cast<const void*>(rotate_kernel), (int)lds);
    hipLaunchKernelGGL(rotate_kernel, dim3((unsigned)row_tiles, (unsigned)splits), dim3(256), lds, (hipStream_t)stream, x, R, (long long)n,
                       d, out);
    WISE_LAUNCH_CHECK("opq rotate_kernel");
    return WISE_OK;
}

extern "C" size_t wise_opq_corr_workspace_bytes(int64_t n, int d) {
    if (n < 0 || !rot_shape_ok(d)) return 0;
    return align_up((size_t)corr_parts(n) * d * d * sizeof(double), 256);
}

extern "C" int wise_opq_corr(const uint8_t* codes, const float* codebooks, const float* x, int64_t n, int d, int m, double* M,
                             void* workspace, size_t workspace_bytes, void* stream) {
    if (!rot_shape_ok(d) || !pq_shape_ok(d, m)) {
        set_error("opq_corr: d=%d m=%d unsupported (d %% 4 == 0, d <= 1024; d %% m == 0, m <= 128, d / m even in [2, 96])", d, m);
        return WISE_E_UNSUPPORTED;
    }
    WISE_CHECK_ARG(n >= 0 && n < (1ll << 15) * CORR_ROWS && M && codebooks && (n == 0 || (codes && x)), "opq_corr: bad argument");
    const size_t need = wise_opq_corr_workspace_bytes(n, d);
    if (!workspace || workspace_bytes < need) {
        set_error("opq_corr: workspace %zu < %zu bytes", workspace_bytes, need);
        return WISE_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int parts = corr_parts(n), tiles = (d + CORR_T - 1) / CORR_T;
    double* P = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(corr_kernel, dim3(tiles, tiles, parts), dim3(256), 0, st, codes, codebooks, x, (long long)n, d, m, P);
    WISE_LAUNCH_CHECK("opq corr_kernel");
    const long long dd = (long long)d * d;
    hipLaunchKernelGGL(corr_fold_kernel, dim3((unsigned)((dd + 255) / 256)), dim3(256), 0, st, P, parts, dd, M);
    WISE_LAUNCH_CHECK("opq corr_fold_kernel");
    return WISE_OK;
}

extern "C" int wise_opq_decode(const uint8_t* codes, int64_t N, const int64_t* pos, int rows, const int64_t* list_off, int nlist,
                               const float* centroids, const float* codebooks, const float* R, int d, int m, float* out, void* stream) {
    if (!rot_shape_ok(d) || !pq_shape_ok(d, m)) {
        set_error("opq_decode: d=%d m=%d unsupported (d %% 4 == 0, d <= 1024; d %% m == 0, m <= 128, d / m even in [2, 96])", d, m);
        return WISE_E_UNSUPPORTED;
    }
    WISE_CHECK_ARG(N >= 0 && rows >= 0 && nlist >= 1 && list_off && centroids && codebooks && R && (N == 0 || codes) &&
                       (rows == 0 || (pos && out)),
                   "opq_decode: bad argument");
    if (rows == 0) return WISE_OK;
    hipLaunchKernelGGL(decode_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, codes, (long long)N, (const long long*)pos,
                       (const long long*)list_off, nlist, centroids, codebooks, R, d, m, out);
    WISE_LAUNCH_CHECK("opq decode_kernel");
    return WISE_OK;
}

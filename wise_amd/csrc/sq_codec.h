// The row codecs and THE SUM OF THE CONTRACT of their scans: what the inverted-list kernels (ivf_sq.hip: IndexIVFSQ8,
// IndexIVFSQfp16) and the flat codec scans (flat_codec_scan.h: IndexSQfp16 and IndexSQfp16L2 over binary16 rows, IndexFlatL2 over fp32 rows) share,
// so that a row's score is the same bits whichever index holds it.
#pragma once
#include "topk_common.h"

namespace wise {

// behind a merge of keys that order -dist (l2_topk.hip): the n outputs D become distances again, the padding +3.4028235e38.
// gate: optional device flag, nothing is done while *gate == 0
int l2_flip_launch(float* D, int n, const int* gate, hipStream_t st);

namespace ivf_sq {

constexpr int SQ_T = 4;                   // wave-loads in flight per wave of the scan

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// s = fmaf(w[4 j + b], (float)byte b of word, s) for b = 0 .. 3: the byte-select conversions, one fma each
__device__ __forceinline__ float chain_word(float s, unsigned word, const float4 w) {
    s = fmaf(w.x, (float)(word & 0xffu), s);
    s = fmaf(w.y, (float)((word >> 8) & 0xffu), s);
    s = fmaf(w.z, (float)((word >> 16) & 0xffu), s);
    s = fmaf(w.w, (float)(word >> 24), s);
    return s;
}

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// s = fmaf(wa, (float)low half of word, s), then s = fmaf(wb, (float)high half, s): binary16 -> fp32 is exact, subnormals kept
__device__ __forceinline__ float chain_halves(float s, unsigned word, float wa, float wb) {
    const f16x2 h = __builtin_bit_cast(f16x2, word);
    s = fmaf(wa, (float)h.x, s);
    s = fmaf(wb, (float)h.y, s);
    return s;
}

// THE CODECS: what a lane (row, c) of the bodies below loads of its row, which 16 weights it holds, and how the two become its
// s_c.  Everything else — the lanes of a wave-load, the fold over the chunks, the list walk, the selection, the range passes — is
// written once and takes the codec as a template parameter; it never branches on it.
//   Codec8   IndexIVFSQ8: d bytes a row.  Chunk c is bytes 16 c .. 16 c + 15, ONE 16-byte load; the weights are W[q, 16 c ..] of
//            wise_sq_query and the score's base is bias + q0.  IndexSQ8bit (ip_sq8.hip) scans the same codes without lists: the
//            same loads, weights and chain, and the base is q0 alone (its policy's score()).
//   Codec16  IndexIVFSQfp16: d binary16 values a row, 2 d bytes = 2 C 16-byte pieces.  Chunk c is piece c and piece c + C, i.e.
//            elements 8 c .. 8 c + 7 (i = 0 .. 7 of the chain) and d / 2 + 8 c .. d / 2 + 8 c + 7 (i = 8 .. 15): each of the TWO
//            load instructions of a wave-load then reads, per row, C consecutive pieces — a contiguous run of d bytes — and whole
//            rows are consumed.  The weights are the query's own values at those elements; there is no q0: base = bias.
struct Codec8 {
    static constexpr int PIECES = 1;
    static __host__ __device__ __forceinline__ size_t row_bytes(int d) { return (size_t)d; }
    static __device__ __forceinline__ float base(float bias, const float* __restrict__ q0, int qi) { return bias + q0[qi]; }
    static __device__ __forceinline__ void weights(const float* __restrict__ wrow, int d, int c, float4 (&w)[4]) {
        const float4* wq = reinterpret_cast<const float4*>(wrow + 16 * c);
        w[0] = wq[0]; w[1] = wq[1]; w[2] = wq[2]; w[3] = wq[3];
    }
    static __device__ __forceinline__ void load(const unsigned char* __restrict__ row, int C, int c, u32x4 (&x)[PIECES]) {
        x[0] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(row) + c);
    }
    static __device__ __forceinline__ float chain(const u32x4 (&x)[PIECES], const float4 (&w)[4]) {
        float a = 0.f;
        a = chain_word(a, x[0][0], w[0]);
        a = chain_word(a, x[0][1], w[1]);
        a = chain_word(a, x[0][2], w[2]);
        a = chain_word(a, x[0][3], w[3]);
        return a;
    }
};

struct Codec16 {
    static constexpr int PIECES = 2;
    static __host__ __device__ __forceinline__ size_t row_bytes(int d) { return (size_t)2 * d; }
    static __device__ __forceinline__ float base(float bias, const float* __restrict__, int) { return bias; }
    static __device__ __forceinline__ void weights(const float* __restrict__ wrow, int d, int c, float4 (&w)[4]) {
        const float4* lo = reinterpret_cast<const float4*>(wrow + 8 * c);
        const float4* hi = reinterpret_cast<const float4*>(wrow + (d >> 1) + 8 * c);
        w[0] = lo[0]; w[1] = lo[1]; w[2] = hi[0]; w[3] = hi[1];
    }
    static __device__ __forceinline__ void load(const unsigned char* __restrict__ row, int C, int c, u32x4 (&x)[PIECES]) {
        x[0] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(row) + c);
        x[1] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(row) + C + c);
    }
    static __device__ __forceinline__ float chain(const u32x4 (&x)[PIECES], const float4 (&w)[4]) {
        float a = 0.f;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            a = chain_halves(a, x[p][0], w[2 * p].x, w[2 * p].y);
            a = chain_halves(a, x[p][1], w[2 * p].z, w[2 * p].w);
            a = chain_halves(a, x[p][2], w[2 * p + 1].x, w[2 * p + 1].y);
            a = chain_halves(a, x[p][3], w[2 * p + 1].z, w[2 * p + 1].w);
        }
        return a;
    }
};

//   CodecL2  IndexFlatL2 (l2_topk.hip) and the lists of IndexIVFFlatL2 (ivf_sq.hip).
//            d fp32 values a row, 4 d bytes = 4 C 16-byte pieces of four floats.  Chunk c is the pieces
//            c, C + c, 2 C + c and 3 C + c, i.e. element i = 0 .. 15 of the chain is e = (i / 4) (d / 4) + 4 c + i % 4: Codec16's
//            load shape with four pieces — each of the FOUR load instructions of a wave-load reads, per row, a contiguous run of
//            d bytes.  The "weights" are the query's own values at those elements and the chain is the squared DISTANCE:
//            t = q[e] - x[e] (one rounded fp32 subtraction), s = fmaf(t, t, s).  No bias; s_0 after the fold is the distance.
struct CodecL2 {
    static constexpr int PIECES = 4;
    static __host__ __device__ __forceinline__ size_t row_bytes(int d) { return (size_t)4 * d; }
    static __device__ __forceinline__ float base(float bias, const float* __restrict__, int) { return bias; }
    static __device__ __forceinline__ void weights(const float* __restrict__ wrow, int d, int c, float4 (&w)[4]) {
#pragma unroll
        for (int p = 0; p < 4; ++p) w[p] = *reinterpret_cast<const float4*>(wrow + p * (d >> 2) + 4 * c);
    }
    static __device__ __forceinline__ void load(const unsigned char* __restrict__ row, int C, int c, u32x4 (&x)[PIECES]) {
#pragma unroll
        for (int p = 0; p < 4; ++p) x[p] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(row) + p * C + c);
    }
    static __device__ __forceinline__ float sq_step(float s, float q, unsigned word) {
        const float t = q - __uint_as_float(word);
        return fmaf(t, t, s);
    }
    static __device__ __forceinline__ float chain(const u32x4 (&x)[PIECES], const float4 (&w)[4]) {
        float a = 0.f;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            a = sq_step(a, w[p].x, x[p][0]);
            a = sq_step(a, w[p].y, x[p][1]);
            a = sq_step(a, w[p].z, x[p][2]);
            a = sq_step(a, w[p].w, x[p][3]);
        }
        return a;
    }
};

//   Codec16L2  IndexSQfp16L2 (l2_sq16.hip): Codec16's rows, load shape and weights — chunk c is piece c and piece c + C, elements
//            8 c .. 8 c + 7 (i = 0 .. 7) and d / 2 + 8 c .. d / 2 + 8 c + 7 (i = 8 .. 15) — under CodecL2's step:
//            t = q[e] - (float)h[e] (the widening is exact, subnormals kept; ONE rounded fp32 subtraction), s = fmaf(t, t, s).
//            No bias; s_0 after the fold is the squared distance.
struct Codec16L2 : Codec16 {
    static __device__ __forceinline__ float sq_halves(float s, unsigned word, float qa, float qb) {
        const f16x2 h = __builtin_bit_cast(f16x2, word);
        const float ta = qa - (float)h.x;
        s = fmaf(ta, ta, s);
        const float tb = qb - (float)h.y;
        return fmaf(tb, tb, s);
    }
    static __device__ __forceinline__ float chain(const u32x4 (&x)[PIECES], const float4 (&w)[4]) {
        float a = 0.f;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            a = sq_halves(a, x[p][0], w[2 * p].x, w[2 * p].y);
            a = sq_halves(a, x[p][1], w[2 * p].z, w[2 * p].w);
            a = sq_halves(a, x[p][2], w[2 * p + 1].x, w[2 * p + 1].y);
            a = sq_halves(a, x[p][3], w[2 * p + 1].z, w[2 * p + 1].w);
        }
        return a;
    }
};

// THE SUM OF THE CONTRACT for SQ_T wave-loads at once (the scan and the range_search kernels): lane (sub, c) reads chunk c of row
// r[t] (an existing row: callers clamp), runs its fmaf chain, and the chunks of a row are folded into its lane c = 0
template <class Codec>
__device__ __forceinline__ void sq_score_loads(const unsigned char* __restrict__ codes, int d, int C, int c, const long long (&r)[SQ_T],
                                               const float4 (&w)[4], float (&s)[SQ_T]) {
    u32x4 x[SQ_T][Codec::PIECES];
#pragma unroll
    for (int t = 0; t < SQ_T; ++t) Codec::load(codes + (size_t)r[t] * Codec::row_bytes(d), C, c, x[t]);
#pragma unroll
    for (int t = 0; t < SQ_T; ++t) s[t] = Codec::chain(x[t], w);
    for (int step = 1; step < C; step <<= 1) {                                      // the chunks of a row: lanes c .. c + C - 1
        const bool take = c + step < C;
#pragma unroll
        for (int t = 0; t < SQ_T; ++t) {
            const float v = __shfl_down(s[t], step, 64);
            s[t] = take ? s[t] + v : s[t];
        }
    }
}

// The same for NQ weight rows that share the loads (the flat scan carries up to 4 queries a pass): s[q][t] is, bit for bit, what
// sq_score_loads gives row r[t] under w[q] — the same chain and the same fold, only the loads are not repeated
template <class Codec, int NQ>
__device__ __forceinline__ void sq_score_loads_nq(const unsigned char* __restrict__ codes, int d, int C, int c, const long long (&r)[SQ_T],
                                                  const float4 (&w)[NQ][4], float (&s)[NQ][SQ_T]) {
    u32x4 x[SQ_T][Codec::PIECES];
#pragma unroll
    for (int t = 0; t < SQ_T; ++t) Codec::load(codes + (size_t)r[t] * Codec::row_bytes(d), C, c, x[t]);
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int t = 0; t < SQ_T; ++t) s[q][t] = Codec::chain(x[t], w[q]);
    for (int step = 1; step < C; step <<= 1) {
        const bool take = c + step < C;
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int t = 0; t < SQ_T; ++t) {
                const float v = __shfl_down(s[q][t], step, 64);
                s[q][t] = take ? s[q][t] + v : s[q][t];
            }
    }
}

}  // namespace ivf_sq
}  // namespace wise

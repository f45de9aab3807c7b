// SVT stages 1 and 2: the fp64 Gram G = Z^T Z of B <= 256 bands on the matrix cores, its fixed-order
// slab reduction (wide cubes too), and the warm start's products A0 = V^T (G V).
#pragma once

#include <utility>

#include "lrs_common.h"
#include "svt_ws.h"

namespace lrs {

// ---- 1. Gram G = Z^T Z on the fp64 matrix cores ---------------------------------------------
// Z = X + c2*L2 (float32: exact in fp64).  One workgroup per slab of rows computes every 16 x 16
// tile pair (a <= b) of the nt = ceil(B/16) column blocks, so Z is read from HBM once: rows are
// staged kGramChunk at a time into LDS with float4 loads (Z formed on the way), then per k-step
// of 4 rows a lane reads Z[p0 + (l>>4)][16c + (l&15)] for all nt blocks (the A and B fragments of
// v_mfma_f64_16x16x4 have that same form) and wave w issues the MFMAs of pairs w, w + 4, ...
// (compile-time pair lists: one instantiation per wave).  Partials [slab][pair][16*16] are
// reduced in fixed order, so G is deterministic.
typedef double doublex4 __attribute__((ext_vector_type(4)));
// NT column blocks (B <= 16 NT) over NW waves: 13 / 4 waves (91 pairs) up to B = 208, 16 / 8 waves
// (136 pairs, 17 accumulators per wave) up to 256
constexpr int kGramChunk = 32;   // rows per LDS chunk (row stride 16 NT + 4)
constexpr int kGramBatch = 13;   // loads in flight per thread

template <int NT>
struct GramPairs {
    int a[gram_npairs(NT)], b[gram_npairs(NT)];
};
template <int NT>
__host__ __device__ constexpr GramPairs<NT> gram_pairs() {
    GramPairs<NT> t{};
    int k = 0;
    for (int a = 0; a < NT; ++a)
        for (int b = a; b < NT; ++b) {
            t.a[k] = a;
            t.b[k] = b;
            ++k;
        }
    return t;
}

template <int NT, int PI>
struct GramPair {
    static constexpr int a = gram_pairs<NT>().a[PI], b = gram_pairs<NT>().b[PI];
};

template <int NT, int NW, int W, int... U>
__device__ __forceinline__ void gram_mfmas(const double (&f)[NT], doublex4 (&acc)[sizeof...(U)],
                                           std::integer_sequence<int, U...>) {
    ((acc[U] = __builtin_amdgcn_mfma_f64_16x16x4f64(f[GramPair<NT, W + NW * U>::a], f[GramPair<NT, W + NW * U>::b],
                                                    acc[U], 0, 0, 0)),
     ...);
}

// Whole workgroup body for wave W (every wave runs the same staging and barriers; the pair list,
// the accumulators and their stores are compile-time per wave, so they stay in registers).
template <int NT, int NW, int W>
__device__ __forceinline__ void gram_body(float *Zs, const float *__restrict__ X, const float *__restrict__ L2,
                                          float c2, int B, int64_t pbeg, int64_t pend, double *__restrict__ out) {
    constexpr int kGramPairs = gram_npairs(NT), kGramLd = 16 * NT + 4, NTH = 64 * NW;
    constexpr int NP = (kGramPairs - W + NW - 1) / NW;
    const int lane = threadIdx.x & 63, g = lane >> 4, jl = lane & 15;
    doublex4 acc[NP];
#pragma unroll
    for (int u = 0; u < NP; ++u) acc[u] = doublex4{0.0, 0.0, 0.0, 0.0};
    for (int64_t c0 = pbeg; c0 < pend; c0 += kGramChunk) {
        const int rows = (int)min<int64_t>(kGramChunk, pend - c0);
        __syncthreads();
        // rows x B elements, kGramBatch loads in flight per thread, then the LDS stores
        for (int e0 = threadIdx.x; e0 < kGramChunk * B; e0 += NTH * kGramBatch) {
            float z[kGramBatch];
#pragma unroll
            for (int u = 0; u < kGramBatch; ++u) {
                const int e = e0 + NTH * u, rr = e / B;
                z[u] = 0.f;
                if (e < kGramChunk * B && rr < rows) {
                    const int64_t o = c0 * B + e;
                    z[u] = X[o];
                    if (L2) z[u] = z[u] + c2 * L2[o];   // X + (1/mu_2)*lambda_2
                }
            }
#pragma unroll
            for (int u = 0; u < kGramBatch; ++u) {
                const int e = e0 + NTH * u, rr = e / B, c = e - rr * B;
                if (e < kGramChunk * B) Zs[rr * kGramLd + c] = z[u];
            }
        }
        for (int idx = threadIdx.x; idx < kGramChunk * (kGramLd - B); idx += NTH) {   // zero pad columns
            const int rr = idx / (kGramLd - B), c = B + idx % (kGramLd - B);
            Zs[rr * kGramLd + c] = 0.f;
        }
        __syncthreads();
        const int rows4 = (rows + 3) & ~3;
        for (int r = 0; r < rows4; r += 4) {
            double f[NT];
#pragma unroll
            for (int c = 0; c < NT; ++c) f[c] = (double)Zs[(r + g) * kGramLd + 16 * c + jl];
            gram_mfmas<NT, NW, W>(f, acc, std::make_integer_sequence<int, NP>{});
        }
    }
    // C/D layout of the f64 MFMA: column l & 15, row (l >> 4) + 4 r
#pragma unroll
    for (int u = 0; u < NP; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(int64_t)(W + NW * u) * 256 + (g + 4 * r) * 16 + jl] = acc[u][r];
}

template <int NT, int NW, int... W>
__device__ __forceinline__ void gram_dispatch(int wv, float *Zs, const float *X, const float *L2, float c2, int B,
                                              int64_t pbeg, int64_t pend, double *out, std::integer_sequence<int, W...>) {
    ((wv == W ? gram_body<NT, NW, W>(Zs, X, L2, c2, B, pbeg, pend, out) : (void)0), ...);
}

template <int NT, int NW>
__global__ __launch_bounds__(64 * NW, 1) void k_gram_mfma(const float *__restrict__ X, const float *__restrict__ L2,
                                                          float c2, int64_t P, int B, int64_t rows_per_slab,
                                                          double *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float Zs[kGramChunk * (16 * NT + 4)];
    const int sl = blockIdx.x, wv = threadIdx.x >> 6;
    const int64_t pbeg = (int64_t)sl * rows_per_slab, pend = min<int64_t>(P, pbeg + rows_per_slab);
    double *out = partial + (int64_t)sl * gram_npairs(NT) * 256;
    gram_dispatch<NT, NW>(wv, Zs, X, L2, c2, B, pbeg, pend, out, std::make_integer_sequence<int, NW>{});
}

// ---- 1b. fixed-order reduction of the slab partials into the full symmetric Gram ------------
__global__ __launch_bounds__(256) void k_gram_reduce16(const double *__restrict__ partial, int nslab, int nt, int B,
                                                       int Bp, double *__restrict__ G) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)Bp * Bp) return;
    const int i = (int)(idx / Bp), j = (int)(idx % Bp);
    if (j < i) return;
    double s = 0.0;
    if (i < B && j < B) {
        const int a = i >> 4, b = j >> 4, npair = gram_npairs(nt);
        const int pi = a * nt - ((a * (a - 1)) >> 1) + (b - a);
        const int e = (i & 15) * 16 + (j & 15);
        double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int sl = 0;
        for (; sl + 8 <= nslab; sl += 8)
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u] += partial[((int64_t)(sl + u) * npair + pi) * 256 + e];
        for (; sl < nslab; ++sl) acc[sl & 7] += partial[((int64_t)sl * npair + pi) * 256 + e];
        s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    }
    G[(int64_t)i * Bp + j] = s;   // pad row/col (B odd) is zero
    G[(int64_t)j * Bp + i] = s;
}

// ---- 2. warm start A0 = V^T (G V) with the current V (16 x 16 fp64 tiles) -------------------
// stage 0: T = G V ; stage 1: A0 = V^T T.  The current V buffer index lives on the device.
__global__ __launch_bounds__(256) void k_gemm_f64_state(SvtWs w, int stage) {
    __shared__ double As[16][17], Bs[16][17];
    const int n = (int)w.Bp;
    const double *V = w.V[w.state[1]];
    const double *A = stage == 0 ? w.G : V;
    const double *Bm = stage == 0 ? V : w.T;
    double *C = stage == 0 ? w.T : w.A0;
    const int ty = threadIdx.x / 16, tx = threadIdx.x % 16;
    const int i = blockIdx.y * 16 + ty, j = blockIdx.x * 16 + tx;
    double acc = 0.0;
    for (int k0 = 0; k0 < n; k0 += 16) {
        const int ka = k0 + tx, kb = k0 + ty;
        if (stage == 1) As[ty][tx] = (i < n && ka < n) ? A[(int64_t)ka * n + i] : 0.0;   // (V^T)[i][ka]
        else As[ty][tx] = (i < n && ka < n) ? A[(int64_t)i * n + ka] : 0.0;
        Bs[ty][tx] = (kb < n && j < n) ? Bm[(int64_t)kb * n + j] : 0.0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) acc = __fma_rn(As[ty][k], Bs[k][tx], acc);
        __syncthreads();
    }
    if (i < n && j < n) C[(int64_t)i * n + j] = acc;
}

}  // namespace lrs

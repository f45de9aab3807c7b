// SVT stage 5: E = V diag(min(tau/s, 1)) V^T after the Jacobi solvers (the tridiagonal chain writes
// its own E), the sorted singular values, and U = Z (I - E) on the f32 matrix cores.
#pragma once

#include <math.h>

#include "lrs_common.h"
#include "svt_eig.h"   // store_fp: the fragment order of F = I - E
#include "svt_ws.h"

namespace lrs {

// ---- 5a. E = V diag(e) V^T, e_k = min(tau/s_k, 1); s_out = sorted singular values -----------
__global__ __launch_bounds__(256) void k_build_E(SvtWs w, int B, double tau) {
    __shared__ double Vi[16][17], Vj[16][17], ek[16];
    const int Bp = (int)w.Bp;
    const double *V = w.V[w.state[1]];
    const int ty = threadIdx.x / 16, tx = threadIdx.x % 16;
    const int i = blockIdx.y * 16 + ty, jrow0 = blockIdx.x * 16;
    const int j = jrow0 + tx;
    double acc = 0.0;
    for (int k0 = 0; k0 < Bp; k0 += 16) {
        Vi[ty][tx] = (i < Bp && k0 + tx < Bp) ? V[(int64_t)i * Bp + k0 + tx] : 0.0;
        Vj[ty][tx] = (jrow0 + ty < Bp && k0 + tx < Bp) ? V[(int64_t)(jrow0 + ty) * Bp + k0 + tx] : 0.0;
        if (threadIdx.x < 16) {
            const int k = k0 + threadIdx.x;
            double e = 0.0;
            if (k < Bp) {
                const double l = w.lam[k];
                const double s = l > 0.0 ? sqrt(l) : 0.0;
                e = (s > tau) ? tau / s : 1.0;
            }
            ek[threadIdx.x] = e;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) acc = __fma_rn(Vi[ty][k] * ek[k], Vj[tx][k], acc);
        __syncthreads();
    }
    if (i < B && j < B) {
        w.E[(int64_t)i * B + j] = (float)acc;
        store_fp(w.Fp, B, i, j, (float)acc);
    }
}

__global__ __launch_bounds__(256) void k_sorted_singular_values(SvtWs w, int B, double *__restrict__ s_out) {
    // rank of each eigenvalue (ties broken by index) -> descending order
    const int Bp = (int)w.Bp;
    for (int i = threadIdx.x; i < Bp; i += blockDim.x) {
        const double li = w.lam[i];
        int rank = 0;
        for (int k = 0; k < Bp; ++k) {
            const double lk = w.lam[k];
            rank += (lk > li) || (lk == li && k < i);
        }
        if (rank < B) s_out[rank] = li > 0.0 ? sqrt(li) : 0.0;
    }
}

// ---- 5b. U = Z (I - E) on the f32 matrix cores --------------------------------------------------
// A wave owns 16 RT rows and the 16 NTL columns from c0 (RT x NTL accumulator tiles) and walks K in
// k-steps of 4.  The k-steps are ordered so that a lane's two A values of k-steps 2q, 2q+1 are one
// aligned float2 of its Z row (k = 8q + 2g + h, lane group g = l >> 4), and F = I - E was written in
// that order by the eigen stage (Fp, store_fp): each B fragment is 64 consecutive floats out of L2.
// No LDS, so several waves per SIMD hide the memory latency; Z is read once per column panel and U
// written once.  Exact f32 products (v_mfma_f32_16x16x4_f32), fp32 accumulation.  Rows >= P, columns
// >= B and k >= B are predicated: nothing is read past a row's end, and rows k >= B of Fp (never
// written: the workspace's zeros) are not read.
// The launched forms (svt_ws.h):
//   <1, 13, 50>, <1, 16, 64>  B <= 256: NST k-steps at compile time (pairs unrolled by 2), every column
//                             in one wave (c0 = 0), grid (ceil(P / 64));
//   <2, 8, 0>                 wide cubes: NST = 0 walks ceil(B / 8) pairs, and the columns are split over
//                             blockIdx.y so that a wave's accumulators stay at 16 tiles (32 rows x 128
//                             columns) however wide the cube is, grid (ceil(P / 128), ceil(B / 128)).
// One __global__ template and no shared device function under two kernels: inlined into a wrapper, the
// same statements give other code in all three forms.
template <int RT, int NTL, int NST>
__global__ __launch_bounds__(256) void k_svt_apply_f(const float *__restrict__ X, const float *__restrict__ L2,
                                                     float c2, const float *__restrict__ Fp, int64_t P, int B,
                                                     float *__restrict__ U) {
    const int lane = threadIdx.x & 63, g = lane >> 4, jl = lane & 15;
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (16 * RT);
    if (r0 >= P) return;
    const int c0 = NST > 0 ? 0 : blockIdx.y * (16 * NTL);
    floatx4 acc[RT][NTL];
#pragma unroll
    for (int m = 0; m < RT; ++m)
#pragma unroll
        for (int t = 0; t < NTL; ++t) acc[m][t] = floatx4{0.f, 0.f, 0.f, 0.f};
    constexpr int kUnroll = NST > 0 ? 2 : 1;
    const int nq = NST > 0 ? NST / 2 : (B + 7) / 8;
#pragma unroll kUnroll
    for (int q = 0; q < nq; ++q) {   // k-steps 2q, 2q + 1
        const int k = 8 * q + 2 * g;
        float2 z[RT];
#pragma unroll
        for (int m = 0; m < RT; ++m) {
            const int64_t row = r0 + 16 * m + jl;
            z[m] = make_float2(0.f, 0.f);
            if (row < P && k < B) {
                if ((B & 1) == 0) {   // even B: 8-byte aligned rows, k + 1 < B
                    z[m] = *reinterpret_cast<const float2 *>(&X[row * B + k]);
                    if (L2) {
                        const float2 l = *reinterpret_cast<const float2 *>(&L2[row * B + k]);
                        z[m].x = z[m].x + c2 * l.x;   // X + (1/mu_2)*lambda_2
                        z[m].y = z[m].y + c2 * l.y;
                    }
                } else {
                    z[m].x = X[row * B + k];
                    if (L2) z[m].x = z[m].x + c2 * L2[row * B + k];
                    if (k + 1 < B) {
                        z[m].y = X[row * B + k + 1];
                        if (L2) z[m].y = z[m].y + c2 * L2[row * B + k + 1];
                    }
                }
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float *fb = Fp + (int64_t)(2 * q + h) * B * 4 + g;
#pragma unroll
            for (int t = 0; t < NTL; ++t) {
                const int c = c0 + 16 * t + jl;
                const float b = (c < B && k + h < B) ? fb[c * 4] : 0.0f;
#pragma unroll
                for (int m = 0; m < RT; ++m) acc[m][t] = mfma16x16x4(h ? z[m].y : z[m].x, b, acc[m][t]);
            }
        }
    }
    // acc[m][t][i] = U[r0 + 16m + 4g + i][c0 + 16t + jl]
#pragma unroll
    for (int m = 0; m < RT; ++m)
#pragma unroll
        for (int t = 0; t < NTL; ++t) {
            const int c = c0 + 16 * t + jl;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t r = r0 + 16 * m + 4 * g + i;
                if (r < P && c < B) U[r * B + c] = acc[m][t][i];
            }
        }
}

}  // namespace lrs

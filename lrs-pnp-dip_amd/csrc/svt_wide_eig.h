// The tridiagonal eigen chain of wide cubes (256 < B <= 512, LRS_SVT_WIDE_TRI): the phases of
// svt_eig.h with their per-lane vectors at 8 registers (lane + 64 t covers 512 columns), and the
// certificate, which at B <= 256 keeps a thread's acc[NB][NB] products in registers, as workspace
// GEMMs on the fp64 matrix cores over many workgroups.  One launch per phase, no host
// synchronisation in between:
// (kernel names below without their k_svt_eig_wide prefix)
//   _tri                       A. G -> packed triangle in w.A0, reduced in place (one workgroup);
//                              with LRS_SVT_WIDE_MW instead n launches of _mw (svt_wide_mw.h): the same
//                              reduction with the trailing matrix's rows over many workgroups
//   _vals, _vecs               B, C. as k_svt_eig_vals / _vecs; residuals and ||T|| -> w.partial
//   _back                      E. V[0] = H_0 ... H_{n-3} W
//   _gemm<false>, _cert        D. S = V^T V -> w.A0 (the packed triangle is dead), then the
//                              certificate's thresholds on S -> state[kWtFlag]
//   3 x (_gemm<true>, _gemm<false>, _cert)
//                              Newton-Schulz V <- V (3I - S)/2 into the other V buffer, the new S and
//                              its check; each returns at once unless the flag asks for a step
//   _fb_jacobi, _fb_vrebuild, _fb_state
//                              the Jacobi chain on the same G when the flag says bad
// then k_build_E from w.V[state[1]] and w.lam, as after the Jacobi chain.  Every sum is taken in a
// fixed order (no floating-point atomics), so reruns are bit-identical.
// The inverse iteration's LU rows (w.F) live at the head of the rotation log (svt_ws.h).
#pragma once

#include "lrs_common.h"
#include "svt_eig.h"
#include "svt_jacobi.h"
#include "svt_ws.h"

namespace lrs {

// state words of the chain (svt_ws.h lists all of them)
constexpr int kWtNs = 5;     // Newton-Schulz steps the last solve ran
constexpr int kWtFlag = 6;   // certificate: kWtDone, kWtStep (one more Newton-Schulz step), kWtBad (fallback)
constexpr int kWtMw = 7;     // 1: the many-workgroup reduction (svt_wide_mw.h) produced the triangle, 0: _tri
constexpr int kWtDone = 0, kWtStep = 1, kWtBad = 2;
constexpr int kWtMaxNs = 3;
constexpr int kWtNv = 8;     // registers of a wave-distributed vector: 64 * 8 = kWideMaxBp columns

__global__ __launch_bounds__(kEigThreads) void k_svt_eig_wide_tri(SvtWs w) {
    extern __shared__ double sm[];   // [n] p vector
    __shared__ double shb[2];
    const int n = (int)w.Bp;
    if (threadIdx.x == 0) w.state[kWtMw] = 0;
    eig_load_packed(w.G, w.A0, n);
    __syncthreads();
    eig_tridiag<true, kWtNv>(w.A0, sm, shb, n, w.beta);
}

__global__ __launch_bounds__(kEigMwThreads) void k_svt_eig_wide_vals(SvtWs w) {
    const int n = (int)w.Bp;
    double gl, gu, tn, pivmin;
    eig_bounds(w.A0, n, gl, gu, tn, pivmin);
    eig_values<kWtNv>(w.A0, n, gl, gu, tn, pivmin, w.lam, w.lam, kEigMwThreads * blockIdx.x);
}

// residuals -> partial[0 .. n - 1], ||T|| (the Gershgorin bound the certificate scales by) -> partial[n]:
// the certificate runs after S has replaced the packed triangle
__global__ __launch_bounds__(kEigMwThreads) void k_svt_eig_wide_vecs(SvtWs w) {
    const int n = (int)w.Bp;
    double gl, gu, tn, pivmin;
    eig_bounds(w.A0, n, gl, gu, tn, pivmin);
    const double r = eig_vectors<kWtNv>(w.A0, w.lam, n, tn, w.F, w.T, kEigMwThreads * blockIdx.x);
    const int i = kEigMwThreads * blockIdx.x + threadIdx.x;
    if (i < n) w.partial[i] = r;
    if (i == 0) w.partial[n] = tn;
}

__global__ __launch_bounds__(256) void k_svt_eig_wide_back(SvtWs w) {
    eig_backtransform<kWtNv>(w.A0, w.beta, (int)w.Bp, w.T, w.V[0], 4 * blockIdx.x, 4 * gridDim.x);
}

// ---- D. the certificate's products on v_mfma_f64_16x16x4 ---------------------------------------
// A workgroup owns a 64 x 64 tile of the n x n result, wave wv its rows 16 wv .. 16 wv + 15 (4
// accumulators); fragments come straight out of L2 (the operands are 2 MB at n = 512).  Lane l
// supplies A[l & 15][l >> 4] and B[l >> 4][l & 15]; it holds C[(l >> 4) + 4 r][l & 15].
//   NS = false: S = V^T V -> w.A0, V = w.V[step & 1] (the basis after `step` Newton-Schulz steps);
//   NS = true:  w.V[step & 1] = 1.5 V - 0.5 V S, V = w.V[(step - 1) & 1], S = w.A0.
// step > 0 runs only while the certificate asks for that step (the flag is kWtStep exactly when the
// previous steps all ran).  Rows, columns and k >= n are predicated.
template <bool NS>
__global__ __launch_bounds__(256) void k_svt_eig_wide_gemm(SvtWs w, int step) {
    typedef double doublex4 __attribute__((ext_vector_type(4)));
    if (step > 0 && w.state[kWtFlag] != kWtStep) return;
    const int n = (int)w.Bp;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, jl = lane & 15;
    const int i0 = blockIdx.y * 64 + 16 * wv, j0 = blockIdx.x * 64;
    if (i0 >= n) return;
    const double *V = w.V[(NS ? step - 1 : step) & 1];
    const double *Bm = NS ? w.A0 : V;
    doublex4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = doublex4{0.0, 0.0, 0.0, 0.0};
    const int i = i0 + jl;
#pragma unroll 4
    for (int k0 = 0; k0 < n; k0 += 4) {
        const int k = k0 + g;
        const bool kok = k < n;
        double a = 0.0, b[4];
        if (kok && i < n) a = NS ? V[(int64_t)i * n + k] : V[(int64_t)k * n + i];   // V(i, k) : V^T(i, k)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = j0 + 16 * t + jl;
            b[t] = (kok && j < n) ? Bm[(int64_t)k * n + j] : 0.0;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[t], acc[t], 0, 0, 0);
    }
    double *C = NS ? w.V[step & 1] : w.A0;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = i0 + g + 4 * r, col = j0 + 16 * t + jl;
            if (row < n && col < n) {
                const int64_t o = (int64_t)row * n + col;
                C[o] = NS ? 1.5 * V[o] - 0.5 * acc[t][r] : acc[t][r];
            }
        }
}

// The thresholds of eig_certify_finish on S = w.A0 (one workgroup; maxima and sums in a fixed order).
// step 0: dev = max |S - I| <= kEigOrth0 and, per vector i, ||T w_i - lambda_i w_i|| +
// 0.5 ||((lambda_j - lambda_i) (S - I)_ji)_j|| <= kEigRes ||T||, else kWtBad; then kWtStep while
// dev > kEigOrth.  step s > 0 (after the s-th Newton-Schulz step and its S): kWtDone once
// dev <= kEigOrth, kWtBad after kWtMaxNs steps.  kWtDone: V valid in buffer s & 1, path 4.
__global__ __launch_bounds__(kEigThreads) void k_svt_eig_wide_cert(SvtWs w, int step) {
    __shared__ double red[kEigThreads / 64], mixs[kEigThreads];
    const int n = (int)w.Bp, tid = threadIdx.x;
    const bool run = step == 0 || w.state[kWtFlag] == kWtStep;
    __syncthreads();   // every thread has read the flag before thread 0 writes it
    if (!run) return;
    const double *S = w.A0;
    double dmax = 0.0;
    for (int e0 = tid; e0 < n * n; e0 += 8 * kEigThreads) {
        double s[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + u * kEigThreads;
            s[u] = e < n * n ? S[e] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + u * kEigThreads, i = e / n, j = e - i * n;
            if (e < n * n) dmax = fmax(dmax, fabs(s[u] - (i == j ? 1.0 : 0.0)));
        }
    }
    for (int off = 32; off > 0; off >>= 1) dmax = fmax(dmax, __shfl_xor(dmax, off, 64));
    if ((tid & 63) == 0) red[tid >> 6] = dmax;
    __syncthreads();
    double dev = 0.0;
    for (int q = 0; q < kEigThreads / 64; ++q) dev = fmax(dev, red[q]);
    bool bad = false;
    if (step == 0) {
        bad = !(dev <= kEigOrth0);
        if (!bad) {
            // column i = tid & 511 of (lambda_j - lambda_i) (S - I)_ji, rows j split in two halves
            const int i = tid & (kWideMaxBp - 1), jh = (n + 1) / 2, jb = (tid >> 9) * jh, je = min(n, jb + jh);
            double mix = 0.0;
            if (i < n) {
                const double li = w.lam[i];
                for (int j0 = jb; j0 < je; j0 += 8) {
                    double s[8], l[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int j = min(j0 + u, je - 1);
                        s[u] = S[(int64_t)j * n + i];
                        l[u] = w.lam[j];
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int j = j0 + u;
                        const double m = (l[u] - li) * (s[u] - (j == i ? 1.0 : 0.0));
                        if (j < je) mix = __fma_rn(m, m, mix);
                    }
                }
            }
            mixs[tid] = mix;
            __syncthreads();
            bool over = false;
            if (tid < kWideMaxBp && i < n) {
                const double bound = w.partial[i] + 0.5 * sqrt(mixs[tid] + mixs[tid + kWideMaxBp]);
                over = !(bound <= kEigRes * w.partial[n]);
            }
            bad = __syncthreads_or(over);
        }
    }
    if (tid == 0) {
        const bool more = !(dev <= kEigOrth);
        const int flag = bad ? kWtBad : !more ? kWtDone : step < kWtMaxNs ? kWtStep : kWtBad;
        w.state[kWtNs] = step;
        w.state[kWtFlag] = flag;
        if (flag == kWtDone) {
            w.state[0] = 1;
            w.state[1] = step & 1;
            w.state[4] = 4;
        }
    }
}

// ---- fallback: the Jacobi chain on the same G, when the certificate refused the basis -----------
// jacobi_core<true> (triangle in w.T, free once the back-transformation has consumed W; the
// rotation log overwrites the dead LU rows), the replay from the identity into w.V[0], the state.
__global__ __launch_bounds__(kJacobiThreads) void k_svt_eig_wide_fb_jacobi(SvtWs w) {
    extern __shared__ double sm[];
    if (w.state[kWtFlag] != kWtBad) return;
    jacobi_core<true>(sm, w, w.G, w.T);
}

__global__ __launch_bounds__(1024) void k_svt_eig_wide_fb_vrebuild(SvtWs w) {
    extern __shared__ double vsm[];
    if (w.state[kWtFlag] != kWtBad) return;
    vrebuild_tile(vsm, w, nullptr, w.V[0], blockIdx.x * vrebuild_rows((int)w.Bp));
}

__global__ void k_svt_eig_wide_fb_state(SvtWs w) {
    if (w.state[kWtFlag] != kWtBad) return;
    w.state[0] = 1;
    w.state[1] = 0;
    w.state[4] = 5;
}

}  // namespace lrs

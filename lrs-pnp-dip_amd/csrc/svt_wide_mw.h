// Phase A of the wide tridiagonal chain over many workgroups (LRS_SVT_WIDE_TRI | LRS_SVT_WIDE_MW,
// 256 < B <= 512): the Householder reduction of svt_eig.h's eig_tridiag with the rows of the trailing
// matrix spread over up to kMwWgs workgroups, one launch per column and the launch boundary as the
// only synchronisation between workgroups (no grid barrier, no flags, no floating-point atomics).
// It leaves w.A0 and w.beta in the form eig_tridiag leaves them (T on the diagonal and the first
// superdiagonal, reflector k in row k from column k + 2 with an implicit leading 1), so
// k_svt_eig_wide_vals and everything after it in svt_wide_eig.h run unchanged.
//
// Launch k = -1, 0, ..., n - 2 of k_svt_eig_wide_mw (n launches; 512 at n = 512), look-ahead form:
//   1. every workgroup reads reflector k (v, beta, and T's d_k, e_k) from the side buffer vbuf[k & 1]
//      and, unless beta = 0, sums the workgroups' partial vectors of column k in workgroup order:
//      p = beta A_sub v, K = beta/2 p.v, w = p - K v.  Same statements on the same data everywhere,
//      so v, w, beta and K are bit-equal in every wave of the grid;
//   2. every wave applies that rank-2 update to the next pivot row k + 1 in registers and forms
//      reflector k + 1 from it (sigma, beta', v': the statements of eig_tridiag).  Nobody writes row
//      k + 1 in this launch: wave 0 of workgroup 0 stores v', beta', e', d' into vbuf[(k + 1) & 1];
//   3. wave 1 of workgroup 0 stores row k of the result (d_k, e_k, v from column k + 2) and beta_k
//      from vbuf[k & 1]: no wave of this launch reads row k.  Launch n - 2 does only this (rows
//      n - 2 and n - 1 of T are then in place) and sets state word kWtMw;
//   4. a wave per row i >= k + 2 (row k + 2 + 8 workgroup + wave, then every kMwRows-th): loads
//      A(i, i..n-1), subtracts v_i w + w_i v (skipped when beta = 0: a column already reduced, e.g.
//      the zero pad of an odd B), stores it, and unless beta' = 0 multiplies it with v' both ways:
//      the row sum goes to element i and A(i, j) v'_i to element j > i of the wave's partial of
//      A_sub v' (the packed triangle holds each off-diagonal element once);
//   5. the waves' partials are added in wave order through LDS and stored as this workgroup's
//      partial vector of column k + 1 (partial buffer (k + 1) & 1).
// Launch -1 reads G instead of the packed triangle (there is no update yet) and stores the rows it
// multiplies into w.A0.  Within a launch no workgroup reads a location another one writes: the pivot
// row and vbuf[k & 1] / partials k & 1 are read-only, rows >= k + 2 belong to one wave each, and row
// k, vbuf[(k + 1) & 1] and partials (k + 1) & 1 are written only.
// The grid of launch k is mw_nwg(n, k) workgroups: the ones that own a row (the host computes it
// from n and k alone; it never reads device state).  Scratch aliases dead workspace (svt_ws.h).
#pragma once

#include "lrs_common.h"
#include "svt_eig.h"
#include "svt_wide_eig.h"
#include "svt_ws.h"

namespace lrs {

constexpr int kMwWgs = 32, kMwThreads = 512, kMwWaves = kMwThreads / 64, kMwRows = kMwWgs * kMwWaves;
static_assert(kMwThreads >= kWideMaxBp, "a thread per column sums the partial vectors");

// workgroups of launch k: those with a row among k + 2 .. n - 1 (workgroup 0 always runs)
__host__ __device__ constexpr int mw_nwg(int n, int k) {
    const int g = (n - (k + 2) + kMwWaves - 1) / kMwWaves;
    return g < 1 ? 1 : g > kMwWgs ? kMwWgs : g;
}
// scratch of column k (svt_ws.h): the workgroups' partials of A_sub v [kMwWgs][n], and reflector k as
// [n] v by absolute column (0 up to column k, 1 at k + 1), then beta_k, e_k, d_k
__device__ __forceinline__ double *mw_part(const SvtWs &w, int k) { return w.partial + (size_t)(k & 1) * kMwWgs * w.Bp; }
__device__ __forceinline__ double *mw_vbuf(const SvtWs &w, int k) { return w.T + (size_t)(k & 1) * (w.Bp + 8); }

__global__ __launch_bounds__(kMwThreads) void k_svt_eig_wide_mw(SvtWs w, int k) {
    __shared__ double ps[kWideMaxBp], qs[kMwWaves][kWideMaxBp];
    const int n = (int)w.Bp, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wg = blockIdx.x;
    const bool first = k < 0, la = k + 1 <= n - 2;   // la: there is a reflector k + 1 (or T's last e) to form
    double *A = w.A0;
    const double *vb = mw_vbuf(w, k);
    const int ip = k + 1;
    // the pivot row as the previous launches left it (in flight while p is summed)
    double x[kWtNv];
    {
        const double *row = first ? w.G : A + (pk_idx(ip, ip, n) - ip);
#pragma unroll
        for (int t = 0; t < kWtNv; ++t) {
            const int j = lane + 64 * t;
            x[t] = (la && j >= ip && j < n) ? row[j] : 0.0;
        }
    }
    // 1. reflector k, p (fixed-order sum of the partials), w = p - K v
    double vj[kWtNv], wj[kWtNv];
#pragma unroll
    for (int t = 0; t < kWtNv; ++t) vj[t] = wj[t] = 0.0;
    const double beta = first ? 0.0 : vb[n];
    if (beta != 0.0) {   // uniform over the grid
        if (tid < n) {
            const double *pp = mw_part(w, k) + tid;
            const int np = mw_nwg(n, k - 1);
            double s = 0.0;
            for (int g0 = 0; g0 < np; g0 += 8) {
                double pg[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) pg[u] = pp[(size_t)min(g0 + u, np - 1) * n];
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (g0 + u < np) s += pg[u];
            }
            ps[tid] = beta * s;
        }
        __syncthreads();
        double kp = 0.0;
#pragma unroll
        for (int t = 0; t < kWtNv; ++t) {
            const int j = lane + 64 * t;
            const int jc = (j < n) ? j : n - 1;
            const double a = vb[jc], pj = ps[jc];
            vj[t] = (j < n) ? a : 0.0;
            wj[t] = (j < n) ? pj : 0.0;
            kp = __fma_rn(wj[t], vj[t], kp);
        }
        const double K = 0.5 * beta * wave_sum_scan(kp);
#pragma unroll
        for (int t = 0; t < kWtNv; ++t) wj[t] = wj[t] - K * vj[t];
    }
    // 2. the updated pivot row and its reflector (every wave; Golub & Van Loan Alg. 5.1.1 as eig_tridiag)
    double vn[kWtNv], betan = 0.0;
#pragma unroll
    for (int t = 0; t < kWtNv; ++t) vn[t] = 0.0;
    if (la) {
        if (beta != 0.0) {
            const double vi = wdist(vj, ip), wi = wdist(wj, ip);
#pragma unroll
            for (int t = 0; t < kWtNv; ++t) {
                const int j = lane + 64 * t;
                if (j >= ip && j < n) x[t] = x[t] - (vi * wj[t] + wi * vj[t]);
            }
        }
        const double dn = wdist(x, ip), x0 = wdist(x, ip + 1);
        double sig = 0.0;
#pragma unroll
        for (int t = 0; t < kWtNv; ++t) {
            const int j = lane + 64 * t;
            const double xs = (j >= ip + 2) ? x[t] : 0.0;
            sig = __fma_rn(xs, xs, sig);
        }
        sig = wave_sum_scan(sig);
        double en = x0, r = 1.0;
        if (sig > 0.0) {
            const double mu = sqrt(__fma_rn(x0, x0, sig));
            const double v1 = (x0 <= 0.0) ? x0 - mu : -sig / (x0 + mu);
            betan = 2.0 * v1 * v1 / (sig + v1 * v1);
            en = mu;
            r = 1.0 / v1;
        }
#pragma unroll
        for (int t = 0; t < kWtNv; ++t) {
            const int j = lane + 64 * t;
            vn[t] = (j == ip + 1) ? 1.0 : (j >= ip + 2) ? x[t] * r : 0.0;   // sigma = 0: the row as it is
        }
        if (wg == 0 && wv == 0) {
            double *vo = mw_vbuf(w, k + 1);
#pragma unroll
            for (int t = 0; t < kWtNv; ++t) {
                const int j = lane + 64 * t;
                if (j < n) vo[j] = vn[t];
            }
            if (lane == 0) {
                vo[n] = betan;
                vo[n + 1] = en;
                vo[n + 2] = dn;
            }
        }
    }
    // 3. row k of the result
    if (!first && wg == 0 && wv == 1) {
        const int rk = pk_idx(k, k, n);
#pragma unroll
        for (int t = 0; t < kWtNv; ++t) {
            const int j = lane + 64 * t;
            if (j >= k + 2 && j < n) A[rk + j - k] = vb[j];
        }
        if (lane == 0) {
            A[rk] = vb[n + 2];
            A[rk + 1] = vb[n + 1];
            if (k < n - 2) w.beta[k] = beta;
            else w.state[kWtMw] = 1;
        }
    }
    // 4. this wave's rows: A_sub -= v w^T + w v^T, then their part of A_sub v'
    const bool mv = la && betan != 0.0;   // uniform over the grid
    double q[kWtNv];
#pragma unroll
    for (int t = 0; t < kWtNv; ++t) q[t] = 0.0;
    for (int i = k + 2 + wg * kMwWaves + wv; i < n; i += kMwRows) {
        const int ri = pk_idx(i, i, n) - i;   // A(i, j) = A[ri + j], j >= i
        const double *row = first ? w.G + (size_t)i * n : A + ri;
        double a[kWtNv];
#pragma unroll
        for (int t = 0; t < kWtNv; ++t) {
            const int j = lane + 64 * t;
            a[t] = (j >= i && j < n) ? row[j] : 0.0;
        }
        if (beta != 0.0) {
            const double vi = wdist(vj, i), wi = wdist(wj, i);
#pragma unroll
            for (int t = 0; t < kWtNv; ++t) {
                const int j = lane + 64 * t;
                if (j >= i && j < n) a[t] = a[t] - (vi * wj[t] + wi * vj[t]);
            }
        }
        if (beta != 0.0 || first) {
#pragma unroll
            for (int t = 0; t < kWtNv; ++t) {
                const int j = lane + 64 * t;
                if (j >= i && j < n) A[ri + j] = a[t];
            }
        }
        if (mv) {
            double s = 0.0;
#pragma unroll
            for (int t = 0; t < kWtNv; ++t) s = __fma_rn(a[t], vn[t], s);   // a = 0 outside the row
            s = wave_sum_scan(s);
            const double vni = wdist(vn, i);
#pragma unroll
            for (int t = 0; t < kWtNv; ++t) {
                const int j = lane + 64 * t;
                q[t] = (j == i) ? q[t] + s : __fma_rn(a[t], vni, q[t]);
            }
        }
    }
    // 5. this workgroup's partial of A_sub v', waves added in order
    if (!mv) return;
#pragma unroll
    for (int t = 0; t < kWtNv; ++t) qs[wv][lane + 64 * t] = q[t];
    __syncthreads();
    if (tid < n) {
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < kMwWaves; ++u) s += qs[u][tid];
        mw_part(w, k + 1)[(size_t)wg * n + tid] = s;
    }
}

}  // namespace lrs

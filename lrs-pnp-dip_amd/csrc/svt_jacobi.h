// SVT stages 3 and 4: the one-workgroup cyclic Jacobi eigensolver on the packed triangle and the
// replay of its rotation log into the eigenvectors.  Launched as kernels of their own (LRS_SVT_JACOBI,
// wide cubes) and called as device functions by the tridiagonal chain's fallback (svt_eig.h).
#pragma once

#include <math.h>

#include "lrs_common.h"
#include "svt_ws.h"

namespace lrs {

constexpr int kJacobiThreads = 1024;

// Workgroup barrier that orders LDS only: waits for this wave's LDS operations (lgkmcnt) but not
// for its outstanding global stores (the rotation log), unlike __syncthreads().
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Round-robin (circle method) pair k of round r over indices 0..Bp-1, returned with p < q.
__device__ __forceinline__ void rr_pair(int r, int k, int Bp, int &p, int &q) {
    if (k == 0) { p = Bp - 1; q = r; }
    else { p = (r + k) % (Bp - 1); q = (r - k + (Bp - 1)) % (Bp - 1); }
    if (p > q) { int t = p; p = q; q = t; }
}

// ---- 3. one-workgroup Jacobi on the packed upper triangle in LDS -----------------------------
// Table-driven: per round the pair indices (ip, iq) and rotations (rc, rs) go to LDS once, the
// packed index of (i <= j) is rowoff[i] + j, and the 2x2 block updates are mapped on a 32 x 32
// thread grid (shifts, no divisions in the inner loop).
// The solve on A = src (packed into LDS, or with GA into Ag in the workspace when the triangle
// exceeds the LDS: B > kLdsMaxBp), eigenvalues to w.lam, rounds/sweeps to w.state[2..3].
template <bool GA>
__device__ __forceinline__ void jac_bar() {
    if (GA) __syncthreads();
    else lds_barrier();
}

template <bool GA>
__device__ __noinline__ void jacobi_core(double *sm, SvtWs w, const double *src, double *Ag = nullptr) {
    const int Bp = (int)w.Bp, half = Bp / 2;
    const int npk = Bp * (Bp + 1) / 2;
    double *A = GA ? Ag : sm;            // packed upper triangle
    double *rc = GA ? sm : A + npk, *rs = rc + half, *red = rs + half;
    int *ip = (int *)(red + 16), *iq = ip + half, *rowoff = iq + half;
    __shared__ int any_rot;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    for (int i = tid; i < Bp; i += kJacobiThreads) rowoff[i] = i * Bp - (i * (i - 1)) / 2 - i;
    __syncthreads();
    for (int i = 0; i < Bp; ++i)
        for (int j = i + tid; j < Bp; j += kJacobiThreads) A[rowoff[i] + j] = src[(int64_t)i * Bp + j];
    __syncthreads();
    int sweeps = 0, rounds = 0;
    // threshold Jacobi: rotate (p,q) only while |a_pq| > tol * sqrt(|a_pp a_qq|); a sweep without
    // any rotation ends the solve (the off-diagonal mass is then below tol relative).
    const double tol = 1e-7;    // residual a_pq perturbs E = f(A) by ~|a_pq| f'(lambda): << 1e-8 relative in U
    while (sweeps < kMaxSweeps) {
        if (tid == 0) any_rot = 0;
        jac_bar<GA>();
        for (int r = 0; r < Bp - 1; ++r) {
            if (tid < half) {
                int p, q;
                rr_pair(r, tid, Bp, p, q);
                const double app = A[rowoff[p] + p], aqq = A[rowoff[q] + q], apq = A[rowoff[p] + q];
                double c = 1.0, s = 0.0;
                if (fabs(apq) > tol * sqrt(fabs(app * aqq)) && apq != 0.0) {
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    c = 1.0 / sqrt(t * t + 1.0);
                    s = t * c;
                    any_rot = 1;
                }
                ip[tid] = p;
                iq[tid] = q;
                rc[tid] = c;
                rs[tid] = s;
                double *log = w.rot + ((int64_t)rounds * half + tid) * 2;
                log[0] = c;
                log[1] = s;
            }
            jac_bar<GA>();
            // A <- J^T A J on every unordered 2x2 block (k1 <= k2); J = [[c, s], [-s, c]] on (p, q).
            // One wave per k1 (wave-uniform rotation), lanes over k2; identity pairs are skipped.
            for (int k1 = wv; k1 < half; k1 += kJacobiThreads / 64) {
                const double c1 = rc[k1], s1 = rs[k1];
                const bool id1 = (s1 == 0.0);
                const int p1 = ip[k1], q1 = iq[k1];
                const int ro_p1 = rowoff[p1], ro_q1 = rowoff[q1];
                for (int k2 = k1 + lane; k2 < half; k2 += 64) {
                    const double c2 = rc[k2], s2 = rs[k2];
                    if (id1 && s2 == 0.0) continue;
                    if (k1 == k2) {
                        const int ipp = ro_p1 + p1, iqq = ro_q1 + q1, ipq = ro_p1 + q1;
                        const double a = A[ipp], b = A[ipq], d = A[iqq];
                        const double la = c1 * a - s1 * b, lb = c1 * b - s1 * d;
                        const double lc = s1 * a + c1 * b, ld = s1 * b + c1 * d;
                        A[ipp] = c1 * la - s1 * lb;
                        A[iqq] = s1 * lc + c1 * ld;
                        A[ipq] = 0.0;
                    } else {
                        const int p2 = ip[k2], q2 = iq[k2];
                        const int i00 = p1 <= p2 ? ro_p1 + p2 : rowoff[p2] + p1;
                        const int i01 = p1 <= q2 ? ro_p1 + q2 : rowoff[q2] + p1;
                        const int i10 = q1 <= p2 ? ro_q1 + p2 : rowoff[p2] + q1;
                        const int i11 = q1 <= q2 ? ro_q1 + q2 : rowoff[q2] + q1;
                        const double a = A[i00], b = A[i01], cc = A[i10], d = A[i11];
                        const double la = c1 * a - s1 * cc, lb = c1 * b - s1 * d;
                        const double lc = s1 * a + c1 * cc, ld = s1 * b + c1 * d;
                        A[i00] = c2 * la - s2 * lb;
                        A[i01] = s2 * la + c2 * lb;
                        A[i10] = c2 * lc - s2 * ld;
                        A[i11] = s2 * lc + c2 * ld;
                    }
                }
            }
            jac_bar<GA>();
            ++rounds;
        }
        ++sweeps;
        const int rotated = any_rot;
        jac_bar<GA>();   // every thread has read the flag before thread 0 resets it
        if (!rotated) break;
    }
    for (int i = tid; i < Bp; i += kJacobiThreads) w.lam[i] = A[rowoff[i] + i];
    if (tid == 0) {
        w.state[2] = rounds;
        w.state[3] = sweeps;
    }
    __syncthreads();   // rotation log and eigenvalues visible to the workgroup (in-kernel fallback)
}

// GA: the triangle in w.T (free here: the warm start's G V product is consumed into A0)
template <bool GA>
__global__ __launch_bounds__(kJacobiThreads) void k_jacobi_lds(SvtWs w, int warm) {
    extern __shared__ double sm[];
    const bool use_warm = warm && w.state[0] == 1;
    jacobi_core<GA>(sm, w, use_warm ? w.A0 : w.G, w.T);
}

// LDS of the solve: the packed triangle (unless GA) + its rotation tables
inline size_t jacobi_lds(int Bp, bool ga) {
    return (ga ? 0 : sizeof(double) * (size_t)Bp * (Bp + 1) / 2) + sizeof(double) * ((size_t)Bp + 16) +
           sizeof(int) * (2 * Bp);
}

// ---- 4. V_new = V_old J_1 ... J_R, vrebuild_rows(Bp) rows per 1024-thread workgroup, rows in LDS
// The rotation log is staged kLogRounds rounds at a time (one global-latency per batch); rounds
// are separated by LDS-only barriers.
constexpr int kLogRounds = 16;

__host__ __device__ constexpr size_t vrebuild_lds(int Bp) {
    return sizeof(double) * ((size_t)vrebuild_rows(Bp) * Bp + (size_t)kLogRounds * (Bp / 2) * 2) +
           sizeof(short) * (size_t)kLogRounds * (Bp / 2) * 2;
}

// Rows i0 .. i0 + vrows - 1 of Vn = Vo J_1 ... J_R (Vo = identity when null); 1024 threads.
__device__ __noinline__ void vrebuild_tile(double *vsm, SvtWs w, const double *Vo, double *Vn, int i0) {
    const int Bp = (int)w.Bp, half = Bp / 2, vrows = vrebuild_rows(Bp);
    double *vrow = vsm;                                   // [vrows][Bp]
    double *lcs = vrow + vrows * Bp;                      // [kLogRounds][half][2]
    short *lpq = (short *)(lcs + kLogRounds * half * 2);  // [kLogRounds][half][2]
    const int nrows = min(vrows, Bp - i0);
    for (int idx = threadIdx.x; idx < nrows * Bp; idx += 1024) {
        const int rr = idx / Bp, j = idx % Bp, i = i0 + rr;
        vrow[rr * Bp + j] = Vo ? Vo[(int64_t)i * Bp + j] : (i == j ? 1.0 : 0.0);
    }
    const int rounds = w.state[2];
    const int rr = threadIdx.x >> 4, kk = threadIdx.x & 15;
    for (int rb = 0; rb < rounds; rb += kLogRounds) {
        const int nr = min(kLogRounds, rounds - rb);
        __syncthreads();
        for (int idx = threadIdx.x; idx < nr * half; idx += 1024) {
            const int ro = idx / half, k = idx % half;
            const double *log = w.rot + ((int64_t)(rb + ro) * half + k) * 2;
            lcs[2 * idx] = log[0];
            lcs[2 * idx + 1] = log[1];
            int p, q;
            rr_pair((rb + ro) % (Bp - 1), k, Bp, p, q);
            lpq[2 * idx] = (short)p;
            lpq[2 * idx + 1] = (short)q;
        }
        __syncthreads();
        for (int ro = 0; ro < nr; ++ro) {
            if (rr < nrows) {
                double *row = vrow + rr * Bp;
                for (int k = kk; k < half; k += 16) {
                    const int e = ro * half + k;
                    const double sn = lcs[2 * e + 1];
                    if (sn == 0.0) continue;
                    const double c = lcs[2 * e];
                    const int p = lpq[2 * e], q = lpq[2 * e + 1];
                    const double vp = row[p], vq = row[q];
                    row[p] = c * vp - sn * vq;
                    row[q] = sn * vp + c * vq;
                }
            }
            lds_barrier();
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < nrows * Bp; idx += 1024) {
        const int r2 = idx / Bp, j = idx % Bp;
        Vn[(int64_t)(i0 + r2) * Bp + j] = vrow[r2 * Bp + j];
    }
}

__global__ __launch_bounds__(1024) void k_jacobi_vrebuild(SvtWs w, int warm) {
    extern __shared__ double vsm[];
    const bool use_warm = warm && w.state[0] == 1;
    const int cur = w.state[1];
    vrebuild_tile(vsm, w, use_warm ? w.V[cur] : nullptr, w.V[cur ^ 1], blockIdx.x * vrebuild_rows((int)w.Bp));
}

__global__ void k_svt_finish_state(SvtWs w) {
    // flip the current-V buffer; V is now valid for warm starts
    w.state[1] ^= 1;
    w.state[0] = 1;
    w.state[4] = 3;
}

}  // namespace lrs

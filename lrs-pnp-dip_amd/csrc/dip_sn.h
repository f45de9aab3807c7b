// DIP low-rank prox, spectral norm: sigma_max of every conv weight (k_sn_gram, k_sn_gram_reduce,
// k_sn_sigma), W_bar / scale (k_sn_apply) and the step head that joins the Gram partials with the first
// conv's weight planes (k_sn_gram_head).  Part of dipnet.hip's translation unit: round_up,
// wave_sum_butterfly and dpp_perm_f64 are lrs_common.h's.
#pragma once
#include <utility>

#include "lrs_common.h"
#include "lrs_dip.h"
#include "dip_wprep.h"   // k_sn_gram_head's conv_prep_body

namespace lrs {

// ------------------------------------------------------------------------------------------
// sigma_max of every conv weight W (rows x cols), batched: one conv per blockIdx.y.
// Gram on the smaller side (m = min(rows, cols) <= 128) in fp64, exact products.
// ------------------------------------------------------------------------------------------
constexpr int kSnMaxDim = 128;
constexpr int kSnSplit = 16;  // inner-dimension split of the Gram (partials reduced by k_sn_gram_reduce; 32: slower)
constexpr int kSnPairs = 36;  // upper 16 x 16 tile pairs of a 128 x 128 Gram
// Gram workspace per conv (doubles): the reduced symmetric Gram [128][128], then the split
// partials [kSnSplit][kSnPairs][16 * 16]
constexpr int64_t kSnGramDoubles = (int64_t)kSnMaxDim * kSnMaxDim + (int64_t)kSnSplit * kSnPairs * 256;

typedef double sn_d4 __attribute__((ext_vector_type(4)));

struct SnPairs {
    int a[kSnPairs], b[kSnPairs];
};
__host__ __device__ constexpr SnPairs sn_pairs() {
    SnPairs t{};
    int k = 0;
    for (int a = 0; a < 8; ++a)
        for (int b = a; b < 8; ++b) {
            t.a[k] = a;
            t.b[k] = b;
            ++k;
        }
    return t;
}

template <int W, int... U>
__device__ __forceinline__ void sn_mfmas(const double (&f)[8], sn_d4 (&acc)[9], std::integer_sequence<int, U...>) {
    constexpr SnPairs P = sn_pairs();
    ((acc[U] = __builtin_amdgcn_mfma_f64_16x16x4f64(f[P.a[W + 4 * U]], f[P.b[W + 4 * U]], acc[U], 0, 0, 0)), ...);
}

// grid (kSnSplit, n), 256 threads: partial z of the 36 upper 16 x 16 tile pairs of the fp64 Gram
// (G = W W^T on the smaller side, m <= 128) over the z-th inner range, on v_mfma_f64_16x16x4
// (exact products of float32 values, fp64 sums).  W is staged 32 inner values at a time in LDS as
// [row][k] floats (row stride 36: the 16 rows x 4 k of a fragment read hit 64 distinct banks); a
// lane's A and B fragments are W[16 c + (l & 15)][k + (l >> 4)] (the same form for both
// operands), wave w owns the pairs w, w + 4, ..., w + 32.
template <int WV>
__device__ __forceinline__ void sn_gram_body(const SnConv &cv, float (*Ws)[36], double *out) {
    const bool rowside = cv.rows <= cv.cols;
    const int m = rowside ? cv.rows : cv.cols;
    const int inner = rowside ? cv.cols : cv.rows;
    const int per = (int)round_up((inner + kSnSplit - 1) / kSnSplit, 32);
    const int kb = blockIdx.x * per, ke = min(inner, kb + per);
    const int t = threadIdx.x, lane = t & 63, g = lane >> 4, jl = lane & 15;
    sn_d4 acc[9];
#pragma unroll
    for (int u = 0; u < 9; ++u) acc[u] = sn_d4{0.0, 0.0, 0.0, 0.0};
    // the next chunk's global loads are issued before this chunk's MFMAs
    float v[16];
    auto load = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int e = t + 256 * u;
            const int r = rowside ? (e >> 5) : (e & 127), kk = rowside ? (e & 31) : (e >> 7);
            const int k = k0 + kk;
            v[u] = (r < m && k < ke) ? (rowside ? cv.W[(int64_t)r * cv.cols + k] : cv.W[(int64_t)k * cv.cols + r]) : 0.f;
        }
    };
    if (kb < ke) load(kb);
    for (int k0 = kb; k0 < ke; k0 += 32) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int e = t + 256 * u;
            const int r = rowside ? (e >> 5) : (e & 127), kk = rowside ? (e & 31) : (e >> 7);
            Ws[r][kk] = v[u];
        }
        __syncthreads();
        if (k0 + 32 < ke) load(k0 + 32);
#pragma unroll
        for (int kq = 0; kq < 32; kq += 4) {
            double f[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) f[c] = (double)Ws[16 * c + jl][kq + g];
            sn_mfmas<WV>(f, acc, std::make_integer_sequence<int, 9>{});
        }
    }
    // C/D layout of the f64 MFMA: column l & 15, row (l >> 4) + 4 r
#pragma unroll
    for (int u = 0; u < 9; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(int64_t)(WV + 4 * u) * 256 + (g + 4 * r) * 16 + jl] = acc[u][r];
}

__global__ __launch_bounds__(256) void k_sn_gram(const SnConv *convs, double *gram) {
    __shared__ float Ws[128][36];
    const SnConv cv = convs[blockIdx.y];
    double *out = gram + (int64_t)blockIdx.y * kSnGramDoubles + (int64_t)kSnMaxDim * kSnMaxDim +
                  (int64_t)blockIdx.x * kSnPairs * 256;
    switch (threadIdx.x >> 6) {
    case 0: sn_gram_body<0>(cv, Ws, out); break;
    case 1: sn_gram_body<1>(cv, Ws, out); break;
    case 2: sn_gram_body<2>(cv, Ws, out); break;
    default: sn_gram_body<3>(cv, Ws, out); break;
    }
}

// grid (kSnPairs, n): tile pair p, element q of its 16 x 16 block (coalesced partial reads): the
// sum over z (in order) of the partials, stored at G[i][j] and mirrored to G[j][i]; G is m x m
// inside the 128 x 128 buffer (the staged rows >= m were zero, so entries outside are 0).
__global__ __launch_bounds__(256) void k_sn_gram_reduce(const SnConv *convs, double *gram) {
    constexpr SnPairs PT = sn_pairs();
    const int p = blockIdx.x, q = threadIdx.x;
    const int i = 16 * PT.a[p] + (q >> 4), j = 16 * PT.b[p] + (q & 15);
    double *G = gram + (int64_t)blockIdx.y * kSnGramDoubles;
    const double *part = G + (int64_t)kSnMaxDim * kSnMaxDim + (int64_t)p * 256 + q;
    double pv[kSnSplit];
#pragma unroll
    for (int z = 0; z < kSnSplit; ++z) pv[z] = part[(int64_t)z * kSnPairs * 256];
    double v = 0.0;
#pragma unroll
    for (int z = 0; z < kSnSplit; ++z) v += pv[z];
    G[i * kSnMaxDim + j] = v;
    if (PT.a[p] != PT.b[p]) G[j * kSnMaxDim + i] = v;
}

// number of eigenvalues of the symmetric tridiagonal T_n above x, T_n given as ab[i] = {alpha_i,
// beta_{i-1}^2}: n minus the sign changes of the characteristic-polynomial sequence p_i =
// (alpha_i - x) p_{i-1} - beta_{i-1}^2 p_{i-2} (division-free; rescaled by a power of two every 4
// terms, which changes no sign).  The sequence starts from p_0 = s0, p_1 = (alpha_0 - x) s0 with s0 =
// sn_scale(top of the round's grid) instead of p_0 = 1: at most 8 unscaled factors then stand between two
// rescalings, the first included (with p_0 = 1 the first rescaling came after 9, which overflowed
// for lambda_max above 1e34 and underflowed to an exact zero below 1e-36).  Signs are the same.
__device__ __forceinline__ double sn_scale(double top) {
    int e;
    const double f = frexp(top, &e);
    (void)f;
    return (top > 0.0 && top < 1e300) ? ldexp(1.0, -e) : 1.0;
}

__device__ __forceinline__ void sturm_term(double a, double b2, double x, double &p, double &pm, int &changes) {
    double pn = __fma_rn(a - x, p, -b2 * pm);
    // a zero takes the sign opposite to its predecessor: perturb it to -p * 2^-600 (the usual
    // Sturm-sequence convention; the next term is then -b2 p (1 + O(2^-600)))
    pn = pn != 0.0 ? pn : -p * 0x1p-600;
    changes += (int)((unsigned long long)(__double_as_longlong(pn) ^ __double_as_longlong(p)) >> 63);
    pm = p;
    p = pn;
}

__device__ __noinline__ int sturm_gt_checked(const double2 *ab, int n, double x, double s0) {
    double pm = s0, p = (ab[0].x - x) * s0;
    p = p != 0.0 ? p : -s0 * 0x1p-600;         // p_0 = s0 > 0: a zero p_1 counts as negative
    int changes = p < 0.0;
    int i = 1;
    double2 c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = ab[min(i + j, kSnMaxDim - 1)];
    for (; i + 4 <= n; i += 4) {
        double2 nx[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) nx[j] = ab[min(i + 4 + j, kSnMaxDim - 1)];
#pragma unroll
        for (int j = 0; j < 4; ++j) sturm_term(c[j].x, c[j].y, x, p, pm, changes);
        int e;
        frexp(fabs(p) > fabs(pm) ? p : pm, &e);
        p = ldexp(p, -e);
        pm = ldexp(pm, -e);
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = nx[j];
    }
    for (; i < n; ++i) sturm_term(ab[i].x, ab[i].y, x, p, pm, changes);
    return n - changes;
}

// The same count with the zero test off the recurrence's dependency chain: the terms are
// evaluated unperturbed and any exact zero is only recorded; a sequence that met one (rare) is
// re-evaluated by sturm_gt_checked.  Without a zero both evaluate the same values (the power-of-
// two rescaling, here every 8 terms, is exact), so the count is the checked one.  Eight terms'
// LDS reads are in flight while eight are evaluated.
__device__ __forceinline__ int sturm_gt(const double2 *ab, int n, double x, double s0) {
    double pm = s0, p = (ab[0].x - x) * s0;
    if (p == 0.0) return sturm_gt_checked(ab, n, x, s0);
    int changes = p < 0.0;
    bool zero = false;
    int i = 1;
    double2 c[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) c[j] = ab[min(i + j, kSnMaxDim - 1)];
    for (; i + 8 <= n; i += 8) {
        double2 nx[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) nx[j] = ab[min(i + 8 + j, kSnMaxDim - 1)];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double pn = __fma_rn(c[j].x - x, p, -c[j].y * pm);
            zero |= pn == 0.0;
            changes += (int)((unsigned long long)(__double_as_longlong(pn) ^ __double_as_longlong(p)) >> 63);
            pm = p;
            p = pn;
        }
        int e;
        frexp(fabs(p) > fabs(pm) ? p : pm, &e);
        p = ldexp(p, -e);
        pm = ldexp(pm, -e);
#pragma unroll
        for (int j = 0; j < 8; ++j) c[j] = nx[j];
    }
    for (; i < n; ++i) {
        const double pn = __fma_rn(ab[i].x - x, p, -ab[i].y * pm);
        zero |= pn == 0.0;
        changes += (int)((unsigned long long)(__double_as_longlong(pn) ^ __double_as_longlong(p)) >> 63);
        pm = p;
        p = pn;
    }
    return zero ? sturm_gt_checked(ab, n, x, s0) : n - changes;
}

// One 256-point multisection round on T_n: thread t tests x_t = base + step (t + 1); returns (to
// every thread) the largest t with an eigenvalue above x_t, or -1.  So the top eigenvalue lies in
// (x_bt, x_{bt+1}] with x_{-1} = base, recomputed by the caller with sn_grid (the same rounding).
// `best` holds 3 slots used round-robin: a round's slot was reset by thread 0 in the previous
// round, before its barrier, and last read two rounds ago.  One barrier per round.
__device__ __forceinline__ double sn_grid(double base, double step, int t) { return base + step * (double)(t + 1); }

// max over the 64 lanes (uniform): DPP row steps, then the four rows' values by readlane
__device__ __forceinline__ int wave_max_i(int v) {
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0x141, 0xF, 0xF, true));   // row_half_mirror
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0x140, 0xF, 0xF, true));   // row_mirror
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

__device__ __forceinline__ int sn_round(const double2 *ab, int n, double base, double step, int *best, int &rnd) {
    const int t = threadIdx.x;
    int *slot = best + rnd % 3;
    if (t == 0) best[(rnd + 1) % 3] = -1;
    // the wave's largest flagged t by DPP, then one LDS atomic per wave (a per-lane atomicMax
    // compiled to a scalar loop over the flagged lanes)
    const double s0 = sn_scale(sn_grid(base, step, 255));
    const int wmax = wave_max_i(sturm_gt(ab, n, sn_grid(base, step, t), s0) >= 1 ? t : -1);
    if ((t & 63) == 0 && wmax >= 0) atomicMax(slot, wmax);
    __syncthreads();
    const int bt = *slot;
    ++rnd;
    return bt;
}

// Narrow [lo, hi] (top eigenvalue inside, lo exclusive) by 257x per round until hi - lo <= tol hi
// (at most 12 rounds: 29 decades; tol >= 1e-12 stays far above the rounding of the grid).
__device__ __forceinline__ void sn_multisect(const double2 *ab, int n, double &lo, double &hi, double tol, int *best,
                                             int &rnd) {
    for (int it = 0; it < 12 && hi - lo > tol * hi; ++it) {
        const double step = (hi - lo) * (1.0 / 257.0);
        const int bt = sn_round(ab, n, lo, step, best, rnd);
        const double nlo = bt >= 0 ? sn_grid(lo, step, bt) : lo;
        const double nhi = bt < 255 ? sn_grid(lo, step, bt + 1) : hi;
        lo = nlo;
        hi = fmax(nlo, nhi);
    }
}

// One workgroup (256 threads) per conv: Lanczos (no reorthogonalisation: the extreme Ritz value
// converges regardless, Paige) with the Gram in registers (thread t holds half a row, 64
// doubles).  The Gershgorin bounds of T_k are kept in registers as rows become final.
// Convergence: at step 24 the top Ritz value is bracketed to a cell of width <= 5e-10 of it
// (multisection from the Gershgorin interval); every 4 steps after that ONE round over the 256
// cells of that width above the bracket's low end relocates it (the top Ritz value only grows
// with k, Cauchy interlacing).  Converged when it stayed in its cell for 4 steps (typically 28-40
// steps for these weights instead of m = 128); one more round then narrows the cell 257x.
// A move of more than 256 cells re-brackets from the Gershgorin bound.
// Guarantee (tests/test_gpu_sigma.py): sigma is within 1 float32 ulp of the fp64 SVD
// value for 5e-20 < sigma < 1e19, unless the top singular vector's component c along the start
// vector is below c(g) for the relative gap g to sigma_2 (c(1e-3) = 3e-8, c(1e-4) = 1e-6, c(1e-5) =
// 3e-5, c(1e-6) = 3e-4; none for g >= 1e-2): the top Ritz value then rests on sigma_2 for 4 steps, the
// rule takes it for converged, and sigma is low by at most the gap (never high).
// sigma32 = float(sqrt(lambda_max)); scale = max(1, sigma32 / ln_lambda) (float32, as torch).
__global__ __launch_bounds__(256) void k_sn_sigma(const SnConv *convs, const double *gram, float *sigma,
                                                  float *scale, float ln_lambda, long long *prof) {
    if (prof && threadIdx.x == 0) prof[blockIdx.x * 8 + 0] = wall_clock64();
    const SnConv cv = convs[blockIdx.x];
    const int m = cv.rows <= cv.cols ? cv.rows : cv.cols;
    const double *G = gram + (int64_t)blockIdx.x * kSnGramDoubles;
    __shared__ __attribute__((aligned(16))) double q[kSnMaxDim];
    __shared__ __attribute__((aligned(16))) double2 ab[kSnMaxDim];   // {alpha_i, beta_{i-1}^2}
    __shared__ int best_s[3];
    // Matvec blocking: thread t holds the 4 x 16 block of G at rows 4 rb .. 4 rb + 3 (rb = t >> 3),
    // columns 16 cb .. 16 cb + 15 (cb = t & 7), so a step reads 16 values of q from LDS per thread
    // (a quarter of what half rows needed: the LDS return bandwidth was the step's largest cost),
    // and the 8 lanes of a row block sum their partials by DPP.  Vector entries: row = 4 rb +
    // (cb & 3), held by lanes cb and cb + 4 (half = cb >> 2; half 0 contributes and writes q).
    // Column chunk c (2 doubles) of a thread is 2 ((c + cb) & 7): the 8 lanes of a row block read
    // distinct LDS banks.
    const int t = threadIdx.x, rb = t >> 3, cb = t & 7, row = 4 * rb + (cb & 3), half = cb >> 2;
    if (t < 3) best_s[t] = -1;
    // the thread's block of the reduced Gram (k_sn_gram_reduce), straight into registers: 32
    // 16-B loads, all in flight.  (No LDS staging: a kernel that asked for the 129 KB a staged
    // copy needs could not start on any CU that held a sparse-coding workgroup, so the DIP
    // stalled at every step's sigma while the sparse coding ran beside it.)
    double g[64];   // g[16 i + 2 c + e] = G[4 rb + i][16 cb + 2 ((c + cb) & 7) + e]
    {
        double2 pv[32];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 8; ++c)
                pv[8 * i + c] = *reinterpret_cast<const double2 *>(G + (int64_t)(4 * rb + i) * kSnMaxDim + 16 * cb +
                                                                   2 * ((c + cb) & 7));
#pragma unroll
        for (int u = 0; u < 32; ++u) {
            g[2 * u] = pv[u].x;
            g[2 * u + 1] = pv[u].y;
        }
    }
    if (prof && t == 0) prof[blockIdx.x * 8 + 1] = wall_clock64();
    int par = 0, rnd = 0;
    // Lanczos on the unnormalised residual r_k (r_0 = start vector): one matvec u' = G r_k, one
    // two-value reduction (||r_k||^2, r_k.u'), then beta_k = ||r_k||, q_k = r_k / beta_k,
    // alpha_k = r_k.u' / beta_k^2 and r_{k+1} = u'/beta_k - alpha_k q_k - beta_k q_{k-1}.
    // Two barriers per step.
    // (Measured: warm-starting from the previous step's top Ritz vector does not shorten the
    // iteration: with Adam at lr 0.1 the weights change by O(their size) every step.)
    double rr = (row < m) ? 1.0 + 0.5 * sin(0.7 * (double)row + 0.3) : 0.0;
    double qprev = 0.0;
    // uniform: Gershgorin max / min over the final rows of T, the last row's alpha and beta
    double gmax = -1e300, gmin = 1e300, a_last = 0.0, b_last = 0.0;
    double blo = 0.0, bhi = 0.0;                  // bracket of the last check's top Ritz value
    bool have = false, converged = false;
    __shared__ double red2[2][8];
    if (half == 0) q[row] = rr;
    __syncthreads();
    int k = 0;
    long long tcheck = 0, ccheck = 0;
    for (; k < m; ++k) {
        // all 8 b128 reads of this thread's 16 entries of q are issued before the first FMA (left
        // to itself the compiler waited on each read)
        double qv[16];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const double2 v = *reinterpret_cast<const double2 *>(q + 16 * cb + 2 * ((c + cb) & 7));
            qv[2 * c] = v.x;
            qv[2 * c + 1] = v.y;
        }
        __builtin_amdgcn_sched_barrier(0);
        double u4[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {   // two independent FMA chains per row
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int c = 0; c < 16; c += 2) {
                s0 = __fma_rn(g[16 * i + c], qv[c], s0);
                s1 = __fma_rn(g[16 * i + c + 1], qv[c + 1], s1);
            }
            u4[i] = s0 + s1;
        }
        // sum over the row block's 8 lanes (xor 1, xor 2, then lane i + lane 7 - i)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            u4[i] += dpp_perm_f64<0xB1>(u4[i]);
            u4[i] += dpp_perm_f64<0x4E>(u4[i]);
            u4[i] += dpp_perm_f64<0x141>(u4[i]);
        }
        const int own = cb & 3;   // (selects, not a branch per lane group)
        const double u01 = (own & 1) ? u4[1] : u4[0], u23 = (own & 1) ? u4[3] : u4[2];
        double u = (own & 2) ? u23 : u01;
        const double w_rr = wave_sum_butterfly(half == 0 ? rr * rr : 0.0);
        const double w_ru = wave_sum_butterfly(half == 0 ? rr * u : 0.0);
        if ((t & 63) == 0) {
            red2[0][(t >> 6) + 4 * par] = w_rr;
            red2[1][(t >> 6) + 4 * par] = w_ru;
        }
        __syncthreads();
        const double s_rr = (red2[0][4 * par] + red2[0][4 * par + 1]) + (red2[0][4 * par + 2] + red2[0][4 * par + 3]);
        const double s_ru = (red2[1][4 * par] + red2[1][4 * par + 1]) + (red2[1][4 * par + 2] + red2[1][4 * par + 3]);
        par ^= 1;
        const double b = sqrt(s_rr);
        if (k > 0 && !(b > 1e-14 * fabs(a_last))) break;   // invariant subspace: T_k is exact
        const double ib = 1.0 / b;
        const double a = s_ru * ib * ib;
        if (t == 0) ab[k] = make_double2(a, s_rr);
        // row k-1 is final now (its off-diagonals beta_{k-1}, beta_k are known); row k so far
        if (k > 0) {
            const double r = b_last + b;
            gmax = fmax(gmax, a_last + r);
            gmin = fmin(gmin, a_last - r);
        }
        a_last = a;
        b_last = k > 0 ? b : 0.0;
        const double qk = rr * ib;
        rr = u * ib - a * qk - (k > 0 ? b : 0.0) * qprev;
        qprev = qk;
        if (k + 1 == m) { ++k; break; }
        if (k + 1 >= 24 && ((k + 1) & 3) == 0) {
            __syncthreads();                      // ab[k] visible
            const long long tc0 = prof ? wall_clock64() : 0, cc0 = prof ? clock64() : 0;
            const int n = k + 1;
            const double ghi = fmax(gmax, a_last + b_last);
            double lo, hi = ghi;
            bool need = true;
            if (have) {
                const double w = bhi - blo;
                const int bt = sn_round(ab, n, blo, w, best_s, rnd);
                if (bt < 0) {
                    converged = true;              // still inside [blo, bhi]
                    need = false;
                } else if (bt < 255) {
                    const double b0 = blo;
                    blo = sn_grid(b0, w, bt);
                    bhi = sn_grid(b0, w, bt + 1);
                    need = false;
                } else {
                    lo = sn_grid(blo, w, 255);
                }
            } else {
                lo = fmax(0.0, fmin(gmin, a_last - b_last));
            }
            if (need) {
                sn_multisect(ab, n, lo, hi, 5e-10, best_s, rnd);
                blo = lo;
                bhi = hi;
                have = true;
            }
            if (prof) { tcheck += wall_clock64() - tc0; ccheck += clock64() - cc0; }
            if (converged) { ++k; break; }
        }
        if (half == 0) q[row] = rr;                   // the matvec reads of q finished before the barrier
        __syncthreads();
    }
    __syncthreads();
    if (prof && t == 0) { prof[blockIdx.x * 8 + 2] = wall_clock64(); prof[blockIdx.x * 8 + 4] = k; prof[blockIdx.x * 8 + 5] = tcheck; prof[blockIdx.x * 8 + 6] = ccheck; }
    double lmax = 0.0;
    if (m > 0) {
        double lo, hi;
        if (converged) {
            // one more round inside the converged cell (width <= 5e-10 lmax -> <= 2e-12)
            lo = blo;
            hi = bhi;
            sn_multisect(ab, k, lo, hi, 0.5 * (bhi - blo) / bhi, best_s, rnd);
        } else {
            // T_k exhausted (k = m) or exact (invariant subspace): from its Gershgorin interval
            lo = fmax(0.0, fmin(gmin, a_last - b_last));
            hi = fmax(gmax, a_last + b_last);
            sn_multisect(ab, k, lo, hi, 1e-12, best_s, rnd);
        }
        lmax = 0.5 * (lo + hi);
    }
    if (prof && t == 0) prof[blockIdx.x * 8 + 3] = wall_clock64();
    if (t == 0) {
        const float s32 = (float)sqrt(fmax(lmax, 0.0));
        sigma[blockIdx.x] = s32;
        scale[blockIdx.x] = fmaxf(1.0f, s32 / ln_lambda);
    }
}

// Wn = W_bar / scale  (all convs; blockIdx.y = conv)
__global__ void k_sn_apply(const SnConv *convs, const float *scale) {
    const SnConv cv = convs[blockIdx.y];
    const int64_t n = (int64_t)cv.rows * cv.cols;
    const float s = scale[blockIdx.y];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        cv.Wn[i] = cv.W[i] / s;
}

}  // namespace lrs

namespace {   // (internal linkage: this header is part of dipnet.hip's translation unit only)

// The step head of the overlapped sigma (StepPlan::sn_overlap): the spectral-norm Gram partials of
// the n convs (blockIdx.y < n, k_sn_gram's body) and, in the extra rows blockIdx.y >= n, the first
// conv's forward planes from the raw weights (the head ConvPrep, dip_wprep.h) with the step's loss
// reset and Adam step count: one launch instead of two.
// kHeadPlaneRows: the first conv's planes on 8 grid rows of kSnSplit workgroups (one row: the kernel took
// 36.7 us, its 16 plane workgroups the longest; 8 rows: 19.2 us, 196^2 step 1.194 -> 1.177 ms, 3 interleaved
// rounds, profiles/r06/ab/head_plane_rows.txt)
constexpr int kHeadPlaneRows = 8;
__global__ __launch_bounds__(256) void k_sn_gram_head(const lrs::SnConv *convs, double *gram, int n,
                                                     const lrs::ConvPrep *head, double *loss_acc, int *step) {
    using namespace lrs;
    __shared__ float Ws[128][36];
    if ((int)blockIdx.y >= n) {   // rows n, n + 1, ...: the planes
        const int64_t b = (int64_t)(blockIdx.y - n) * gridDim.x + blockIdx.x;
        if (b == 0 && threadIdx.x == 0) {   // a training step begins
            *loss_acc = 0.0;
            *step += 1;
        }
        conv_prep_body(*head, 1.0f, b * blockDim.x + threadIdx.x, (int64_t)(gridDim.y - n) * gridDim.x * blockDim.x);
        return;
    }
    const SnConv cv = convs[blockIdx.y];
    double *out = gram + (int64_t)blockIdx.y * kSnGramDoubles + (int64_t)kSnMaxDim * kSnMaxDim +
                  (int64_t)blockIdx.x * kSnPairs * 256;
    switch (threadIdx.x >> 6) {
    case 0: sn_gram_body<0>(cv, Ws, out); break;
    case 1: sn_gram_body<1>(cv, Ws, out); break;
    case 2: sn_gram_body<2>(cv, Ws, out); break;
    default: sn_gram_body<3>(cv, Ws, out); break;
    }
}

}  // namespace

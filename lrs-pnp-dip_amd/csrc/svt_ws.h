// SVT low-rank prox: the shape classes (which kernel forms serve which band count) and the
// workspace every stage works in.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "svt_wide.h"

namespace lrs {

constexpr int kGramSlabs = 256;
// The packed fp64 triangle of 198 x 198 = 157,608 B fits the LDS beside the solver's vectors and
// flags (at Bp = 200 the chain would need 164,128 B > 160 KiB): up to kLdsMaxBp the one-workgroup
// chain keeps it in LDS; above (the 224-band cubes of BASELINE configs[3]/[4]) the same chain runs
// on the packed triangle in the workspace (L2-resident: 224^2/2 x 8 B = 200 KB), with full
// workgroup barriers instead of LDS-only ones.  kMaxBp: every phase's register / lane layout;
// above it, up to kWideMaxBp (svt_wide.h), the wide-band path: tiled Gram and apply kernels around
// the Jacobi chain on the workspace triangle (1 MB at Bp = 512).
constexpr int kLdsMaxBp = 198;
constexpr int kMaxBp = 256;
constexpr int kMaxSweeps = 40;

__host__ __device__ constexpr int gram_npairs(int nt) { return nt * (nt + 1) / 2; }

// ---- shape classes ----------------------------------------------------------------------------
// The launched forms per band count B (Bp = B rounded up to even).  Every launch site, LDS size and
// workspace extent that depends on the band count reads it here.
struct SvtShape {
    bool wide;      // k_gram_wide, the Jacobi chain (or, LRS_SVT_WIDE_TRI, svt_wide_eig.h's), the apply over column panels
    bool ga;        // the solvers' packed triangle in the workspace (global A), not in LDS
    int gram_nt;    // 16-column blocks of the Gram partials; B <= kMaxBp: k_gram_mfma<gram_nt, gram_nw>
    int gram_nw;    //   its waves per workgroup
    int ap_rt;      // k_svt_apply_f<ap_rt, ap_ntl, ap_nst>: 16-row tiles per wave,
    int ap_ntl;     //   16-column tiles per wave (wide: per column panel of the grid),
    int ap_nst;     //   compile-time k-steps of 4 (0: the kernel walks ceil(B / 8) pairs)
    int fp_steps;   // k-steps of 4 that Fp holds
    int nb;         // k_svt_eig<nb, ga> / k_svt_eig_cert<nb, ga>: 32-blocks of the fp64 products (0: none)
    int vrows;      // rows of V per workgroup of the replay (k_jacobi_vrebuild): what fits the LDS
};

__host__ __device__ constexpr SvtShape svt_shape(int Bp, int B) {
    //                           wide   ga     Gram    apply      Fp  nb  vrows
    if (Bp <= kLdsMaxBp) return {false, false, 13, 4,  1, 13, 50, 50, 7,  64};
    if (B <= 200)        return {false, true,  13, 4,  1, 13, 50, 50, 7,  32};
    if (B <= 208)        return {false, true,  13, 4,  1, 16, 64, 64, 7,  32};
    if (Bp <= 224)       return {false, true,  16, 8,  1, 16, 64, 64, 7,  32};
    if (Bp <= kMaxBp)    return {false, true,  16, 8,  1, 16, 64, 64, 8,  32};
    // 256 < Bp <= kWideMaxBp; at Bp = 512 the replay's 16 rows are 65,536 B beside 81,920 B of staged log
    return {true, true, (B + 15) / 16, 4, kWideApRows, kWideApTiles, 0, wide_ap_steps(B), 0, 16};
}
__host__ __device__ constexpr SvtShape svt_shape(int64_t B) { return svt_shape((int)(B + (B & 1)), (int)B); }
// the kernels know Bp only; vrows is the same for both band counts of a Bp
__host__ __device__ constexpr int vrebuild_rows(int Bp) { return svt_shape(Bp, Bp).vrows; }

// ---- workspace --------------------------------------------------------------------------------
struct SvtWs {
    double *partial;  // [kGramSlabs, wide kWideSlabs][16x16 tile pairs][256]  Gram partials
    double *G;        // [Bp][Bp]
    double *A0;       // [Bp][Bp]  V^T G V (warm start)
    double *T;        // [Bp][Bp]  scratch
    double *V[2];     // [Bp][Bp]  eigenvectors, double-buffered
    double *lam;      // [Bp]      eigenvalues (diag of the converged A)
    double *rot;      // [kMaxSweeps*(Bp-1)][Bp/2][2]  (c, s) per round and pair (84 MB at Bp = 512)
    double *beta;     // [Bp]      Householder scalars (tridiagonal path)
    double *F;        // [Bp][4][Bp] pivoted LU rows of T - lambda_i I (inverse iteration; wide: the head of rot)
    float *E;         // [B][B]
    float *Fp;        // [fp_steps][B][4]  I - E in the apply kernels' fragment order
    int *state;       // [0] V valid, [1] current V buffer, [2] rounds, [3] sweeps,
                      // [4] path of the last solve (1 tridiagonal, 2 Jacobi fallback, 3 Jacobi, 4 wide
                      // tridiagonal, 5 its Jacobi fallback), [5] Newton-Schulz steps and [6] certificate
                      // flag of the wide tridiagonal chain (svt_wide_eig.h), [7] 1 when that chain's triangle
                      // came from the many-workgroup reduction (svt_wide_mw.h)
    int64_t Bp;
};

// Byte offsets of the arrays above from the workspace base (each 256-aligned), in this order, and
// the size to allocate.  They depend on the band count alone.
// Wide cubes have no F region of their own: their tridiagonal chain's F (4 Bp^2 doubles: 2.1 MB at
// Bp = 258, 8.4 MB at 512) is the head of rot (kMaxSweeps (Bp - 1) (Bp / 2) 16 B: 21 MB and 84 MB).
// F is written and read by the inverse iteration alone and is dead before the chain's Jacobi
// fallback, the only writer of the rotation log in that call, starts.
// The many-workgroup Householder reduction (LRS_SVT_WIDE_MW, svt_wide_mw.h) has no region either.  It
// runs between k_gram_reduce16 and k_svt_eig_wide_vals and takes
//   * the head of partial, 2 x kMwWgs x Bp doubles (256 KB at Bp = 512 of >= 10 MB), for the
//     workgroups' partial vectors of A_sub v, double-buffered by column parity: the Gram partials are
//     dead once k_gram_reduce16 has written G, and partial[0 .. Bp] (residuals, ||T||) is next
//     written by k_svt_eig_wide_vecs, after the reduction's last launch;
//   * the head of T, 2 x (Bp + 8) doubles, for the reflector in flight (v, beta, e, d), also by
//     column parity: T is unused until k_svt_eig_wide_vecs writes W into it.
struct SvtWsOffsets {
    size_t state, partial, G, A0, T, V[2], lam, rot, beta, F, Fp, E, total;
};

inline SvtWsOffsets svt_ws_offsets(int64_t B) {
    const size_t Bp = (size_t)(B + (B & 1));
    const SvtShape sh = svt_shape(B);
    size_t p = 0;
    auto take = [&](size_t bytes) {
        const size_t r = p;
        p += (bytes + 255) / 256 * 256;
        return r;
    };
    const size_t mat = Bp * Bp * sizeof(double);
    const size_t tiles = (size_t)(sh.wide ? kWideSlabs : kGramSlabs) * gram_npairs(sh.gram_nt);
    SvtWsOffsets o;
    o.state = take(256);
    o.partial = take(tiles * 256 * sizeof(double));
    o.G = take(mat);
    o.A0 = take(mat);
    o.T = take(mat);
    o.V[0] = take(mat);
    o.V[1] = take(mat);
    o.lam = take(Bp * sizeof(double));
    o.rot = take((size_t)kMaxSweeps * (Bp - 1) * (Bp / 2) * 2 * sizeof(double));
    o.beta = take(Bp * sizeof(double));
    o.F = sh.wide ? o.rot : take(4 * mat);
    o.Fp = take((size_t)sh.fp_steps * B * 4 * sizeof(float));
    o.E = p;
    o.total = o.E + (size_t)B * B * sizeof(float) + 256;
    return o;
}

inline SvtWs svt_ws_layout(void *base, int64_t B) {
    const SvtWsOffsets o = svt_ws_offsets(B);
    char *b = (char *)base;
    SvtWs w;
    w.partial = (double *)(b + o.partial);
    w.G = (double *)(b + o.G);
    w.A0 = (double *)(b + o.A0);
    w.T = (double *)(b + o.T);
    w.V[0] = (double *)(b + o.V[0]);
    w.V[1] = (double *)(b + o.V[1]);
    w.lam = (double *)(b + o.lam);
    w.rot = (double *)(b + o.rot);
    w.beta = (double *)(b + o.beta);
    w.F = (double *)(b + o.F);
    w.E = (float *)(b + o.E);
    w.Fp = (float *)(b + o.Fp);
    w.state = (int *)(b + o.state);
    w.Bp = B + (B & 1);
    return w;
}

}  // namespace lrs

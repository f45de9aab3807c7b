// SVT low-rank prox: U = SVT(Z, tau), Z = X + c2*L2 (main_LRS_PnP.py:112-124, called at :315 as
// SVT(X + (1/mu_2)*lambda_2, 1/mu_2)).
//
// The reference runs a float32 LAPACK SVD of the P x B matrix.  Here, MI355X-first:
//   1. fp64 Gram G = Z^T Z over row slabs (many workgroups, coalesced rows), fixed-order reduce;
//   2. warm start: A0 = V^T G V with the previous outer iteration's eigenvectors (tiled fp64
//      GEMMs) — nearly diagonal, so Jacobi needs 1-3 sweeps instead of ~8;
//   3. ONE workgroup runs a cyclic parallel (round-robin) two-sided Jacobi on A held in LDS as a
//      packed fp64 upper triangle (B <= 198: <= 157,608 B), logging each round's rotations;
//   4. the eigenvector update V <- V J_1 ... J_R is replayed from the log row by row in parallel
//      (rows of V evolve independently), off the Jacobi workgroup's critical path;
//   3'. by default, instead of 2-4: ONE workgroup runs a tridiagonal eigensolver with a certificate
//      and 3-4 as its fallback, and writes E itself;
//   5. E = V diag(min(tau/s, 1)) V^T (fp64 -> f32) and U = Z - Z E.
//      Z V diag((s-tau)_+/s) V^T == U_s (S-tau)_+ V_h, and E is small so its f32 rounding costs
//      << 1e-6 relative in U.
// The whole chain runs on its own stream beside the sparse-coding kernel.
// Wide cubes (256 < B <= 512, svt_wide.h): 1 and 5 are tiled over column panels, and 2-4 run on the
// packed triangle in the workspace whatever solver the caller asked for, unless LRS_SVT_WIDE_TRI asks
// for 3' over many workgroups with its certificate as GEMMs on the fp64 matrix cores (svt_wide_eig.h);
// LRS_SVT_WIDE_MW beside it spreads that chain's Householder reduction over many workgroups too, one
// launch per column (svt_wide_mw.h).
//
// The stages: svt_gram.h (1, 2), svt_jacobi.h (3, 4), svt_eig.h (3'), svt_apply.h (5), svt_wide.h (the
// wide Gram), svt_wide_eig.h (the wide 3'), svt_wide_mw.h (its many-workgroup reduction); svt_ws.h has
// the workspace and the table of which form serves which band count.  Here: the launchers and the C entry points.
#include <algorithm>

#include "lrs_common.h"
#include "svt_apply.h"
#include "svt_eig.h"
#include "svt_gram.h"
#include "svt_jacobi.h"
#include "svt_wide.h"
#include "svt_wide_eig.h"
#include "svt_wide_mw.h"
#include "svt_ws.h"

using namespace lrs;

typedef void (*GramKernel)(const float *, const float *, float, int64_t, int, int64_t, double *);
typedef void (*ApplyKernel)(const float *, const float *, float, const float *, int64_t, int, float *);
typedef void (*JacobiKernel)(SvtWs, int);
typedef void (*TriKernel)(SvtWs);
typedef void (*EigKernel)(SvtWs, int, double);

// The instantiations behind a shape class (null: the class does not launch that stage's template).
// Each pointer serves hipFuncSetAttribute and the launch alike.
struct SvtKernels {
    GramKernel gram;       // k_gram_mfma<gram_nt, gram_nw>; wide: k_gram_wide, launched by name
    JacobiKernel jacobi;   // k_jacobi_lds<ga>
    TriKernel tri;         // k_svt_eig_tri<ga>
    EigKernel eig, cert;   // k_svt_eig<nb, ga>, k_svt_eig_cert<nb, ga>
    ApplyKernel apply;     // k_svt_apply_f<ap_rt, ap_ntl, ap_nst>
};

static SvtKernels svt_kernels(const SvtShape &s) {
    SvtKernels k{};
    k.jacobi = s.ga ? k_jacobi_lds<true> : k_jacobi_lds<false>;
    if (s.wide) {
        k.apply = k_svt_apply_f<kWideApRows, kWideApTiles, 0>;
        return k;
    }
    k.gram = s.gram_nt == 13 ? k_gram_mfma<13, 4> : k_gram_mfma<16, 8>;
    k.tri = s.ga ? k_svt_eig_tri<true> : k_svt_eig_tri<false>;
    k.eig = s.nb == 8 ? k_svt_eig<8, true> : s.ga ? k_svt_eig<7, true> : k_svt_eig<7, false>;
    k.cert = s.nb == 8 ? k_svt_eig_cert<8, true> : s.ga ? k_svt_eig_cert<7, true> : k_svt_eig_cert<7, false>;
    k.apply = s.ap_ntl == 13 ? k_svt_apply_f<1, 13, 50> : k_svt_apply_f<1, 16, 64>;
    return k;
}

extern "C" size_t lrs_svt_workspace(int64_t P, int64_t B) {
    if (P <= 0 || B <= 0) return 0;
    return svt_ws_offsets(B).total;
}

extern "C" int64_t lrs_svt_max_bands(void) { return kWideMaxBp; }

// Above kMaxBp the wide-band path serves, up to kWideMaxBp; it has no multi-workgroup solver.
static int svt_shape_check(int64_t B, int warm) {
    const int64_t Bp = B + (B & 1);
    if (Bp > kWideMaxBp) return LRS_E_UNSUPPORTED;
    if (Bp > kMaxBp && (warm & LRS_SVT_MULTI_WG)) return LRS_E_UNSUPPORTED;
    return LRS_OK;
}

// The wide tridiagonal chain (svt_wide_eig.h) serves; an explicit LRS_SVT_JACOBI wins.
static bool svt_wide_tri(int64_t B, int warm) {
    return svt_shape(B).wide && (warm & LRS_SVT_WIDE_TRI) && !(warm & LRS_SVT_JACOBI);
}
// The flag word as the launchers read it: LRS_SVT_WIDE_TRI means something above kMaxBp only, and
// LRS_SVT_WIDE_MW only where the wide tridiagonal chain serves.
static int svt_flags(int64_t B, int warm) {
    if (!svt_shape(B).wide) warm &= ~LRS_SVT_WIDE_TRI;
    return svt_wide_tri(B, warm) ? warm : warm & ~LRS_SVT_WIDE_MW;
}

extern "C" int lrs_svt_gram_offset(int64_t P, int64_t B, int64_t *offset_bytes, int64_t *ld) {
    if (P <= 0 || B <= 0 || !offset_bytes || !ld) return LRS_E_INVALID;
    if (B + (B & 1) > kMaxBp) return LRS_E_UNSUPPORTED;
    *offset_bytes = (int64_t)svt_ws_offsets(B).G;
    *ld = B + (B & 1);
    return LRS_OK;
}

// Stage 1 (multi-workgroup): fp64 Gram on the matrix cores and, for a warm Jacobi, A0 = V^T G V.
extern "C" int lrs_svt_gram_f32(const float *X, const float *L2, float c2, int64_t P, int64_t B, int warm, void *ws,
                                size_t ws_bytes, void *stream) {
    if (!X || !ws || P <= 0 || B <= 0) return LRS_E_INVALID;
    if (svt_shape_check(B, warm) != LRS_OK) return LRS_E_UNSUPPORTED;
    if (ws_bytes < svt_ws_offsets(B).total) return LRS_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    SvtWs w = svt_ws_layout(ws, B);
    const bool wide_tri = svt_wide_tri(B, warm);
    warm = svt_flags(B, warm);
    if (!warm || (wide_tri && !(warm & LRS_SVT_WARM))) {
        hipError_t e = hipMemsetAsync(w.state, 0, sizeof(int) * 8, st);   // words 0-3, and 4-7 (every solve rewrites 4-6)
        if (e != hipSuccess) return (int)e;
    }
    const int Bp = (int)w.Bp;
    const SvtShape sh = svt_shape(B);
    const int slabs = sh.wide ? kWideSlabs : kGramSlabs;
    int64_t rows = ((P + slabs - 1) / slabs + 3) / 4 * 4;
    const int nslab = (int)((P + rows - 1) / rows);
    if (sh.wide) {
        const int npan = wide_npanels((int)B);
        hipLaunchKernelGGL(k_gram_wide, dim3((unsigned)nslab, (unsigned)(npan * (npan + 1) / 2)), dim3(256), 0, st, X,
                           L2, c2, P, (int)B, rows, sh.gram_nt, w.partial);
    } else {
        hipLaunchKernelGGL(svt_kernels(sh).gram, dim3((unsigned)nslab), dim3(64 * sh.gram_nw), 0, st, X, L2, c2, P,
                           (int)B, rows, w.partial);
    }
    LRS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_gram_reduce16, dim3((unsigned)((Bp * Bp + 255) / 256)), dim3(256), 0, st, w.partial, nslab,
                       sh.gram_nt, (int)B, Bp, w.G);
    LRS_CHECK_LAUNCH();
    if ((warm & LRS_SVT_WARM) && ((warm & LRS_SVT_JACOBI) || sh.wide) && !wide_tri) {
        // A0 = V^T (G V) with the current V (unused when V is not valid yet: Jacobi starts from G)
        const dim3 g16((Bp + 15) / 16, (Bp + 15) / 16);
        hipLaunchKernelGGL(k_gemm_f64_state, g16, dim3(256), 0, st, w, 0);
        LRS_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_gemm_f64_state, g16, dim3(256), 0, st, w, 1);
        LRS_CHECK_LAUNCH();
    }
    return LRS_OK;
}

// U = Z (I - E) from the F = I - E the eigen stage left in w.Fp: the apply kernel of this band count
static int svt_apply(const float *X, const float *L2, float c2, int64_t P, int64_t B, const SvtWs &w, float *U,
                     hipStream_t st) {
    const SvtShape sh = svt_shape(B);
    const int64_t rows = 64 * sh.ap_rt, panel = 16 * sh.ap_ntl;   // per workgroup; every column unless wide
    const dim3 grid((unsigned)((P + rows - 1) / rows), sh.wide ? (unsigned)((B + panel - 1) / panel) : 1u);
    hipLaunchKernelGGL(svt_kernels(sh).apply, grid, dim3(256), 0, st, X, L2, c2, w.Fp, P, (int)B, U);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// Stage 2: one-workgroup eigensolver (runs beside the sparse-coding kernel), E, U.
extern "C" int lrs_svt_finish_f32(const float *X, const float *L2, float c2, int64_t P, int64_t B, double tau,
                                  float *U, double *s_out, int warm, void *ws, size_t ws_bytes, void *stream) {
    if (!X || !U || !ws || P <= 0 || B <= 0 || tau < 0.0) return LRS_E_INVALID;
    if (svt_shape_check(B, warm) != LRS_OK) return LRS_E_UNSUPPORTED;
    if (ws_bytes < svt_ws_offsets(B).total) return LRS_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    SvtWs w = svt_ws_layout(ws, B);
    const int Bp = (int)w.Bp;
    const SvtShape sh = svt_shape(B);
    const SvtKernels k = svt_kernels(sh);
    // dynamic LDS above 64 KiB must be opted into; request exactly what this shape needs
    auto opt_in = [](const void *kernel, size_t bytes) {
        return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    };
    const size_t smem = jacobi_lds(Bp, sh.ga);
    const size_t vsmem = vrebuild_lds(Bp);
    const bool wide_tri = svt_wide_tri(B, warm);
    warm = svt_flags(B, warm);
    if (wide_tri) {
        // tridiagonalisation, eigenvalues, inverse iteration, back-transformation; S = V^T V and its
        // certificate, kWtMaxNs gated Newton-Schulz steps, the gated Jacobi fallback; then E as below
        hipError_t ea = opt_in((const void *)k_svt_eig_wide_fb_vrebuild, vsmem);
        if (ea != hipSuccess) return (int)ea;
        const dim3 g64((unsigned)((Bp + 63) / 64), (unsigned)((Bp + 63) / 64));
        if (warm & LRS_SVT_WIDE_MW) {
            // the reduction over many workgroups: launch k forms reflector k + 1 and applies reflector k
            for (int kc = -1; kc <= Bp - 2; ++kc) {
                hipLaunchKernelGGL(k_svt_eig_wide_mw, dim3((unsigned)mw_nwg(Bp, kc)), dim3(kMwThreads), 0, st, w, kc);
                LRS_CHECK_LAUNCH();
            }
        } else {
            hipLaunchKernelGGL(k_svt_eig_wide_tri, dim3(1), dim3(kEigThreads), sizeof(double) * Bp, st, w);
            LRS_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(k_svt_eig_wide_vals, dim3((unsigned)((4 * Bp + kEigMwThreads - 1) / kEigMwThreads)),
                           dim3(kEigMwThreads), 0, st, w);
        LRS_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_svt_eig_wide_vecs, dim3((unsigned)((Bp + kEigMwThreads - 1) / kEigMwThreads)),
                           dim3(kEigMwThreads), 0, st, w);
        LRS_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_svt_eig_wide_back, dim3((unsigned)((Bp + 15) / 16)), dim3(256), 0, st, w);
        LRS_CHECK_LAUNCH();
        for (int step = 0; step <= kWtMaxNs; ++step) {
            if (step > 0) {
                hipLaunchKernelGGL(k_svt_eig_wide_gemm<true>, g64, dim3(256), 0, st, w, step);
                LRS_CHECK_LAUNCH();
            }
            hipLaunchKernelGGL(k_svt_eig_wide_gemm<false>, g64, dim3(256), 0, st, w, step);
            LRS_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_svt_eig_wide_cert, dim3(1), dim3(kEigThreads), 0, st, w, step);
            LRS_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(k_svt_eig_wide_fb_jacobi, dim3(1), dim3(kJacobiThreads), smem, st, w);
        LRS_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_svt_eig_wide_fb_vrebuild, dim3((unsigned)((Bp + sh.vrows - 1) / sh.vrows)), dim3(1024),
                           vsmem, st, w);
        LRS_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_svt_eig_wide_fb_state, dim3(1), dim3(1), 0, st, w);
        LRS_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_build_E, dim3((unsigned)((B + 15) / 16), (unsigned)((B + 15) / 16)), dim3(256), 0, st,
                           w, (int)B, tau);
        LRS_CHECK_LAUNCH();
    } else if (sh.wide || (warm & LRS_SVT_JACOBI)) {   // wide: the Jacobi chain unless LRS_SVT_WIDE_TRI asks
        const int jwarm = warm & LRS_SVT_WARM;
        hipError_t ea = opt_in((const void *)k.jacobi, smem);
        if (ea == hipSuccess) ea = opt_in((const void *)k_jacobi_vrebuild, vsmem);
        if (ea != hipSuccess) return (int)ea;
        hipLaunchKernelGGL(k.jacobi, dim3(1), dim3(kJacobiThreads), smem, st, w, jwarm);
        LRS_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_jacobi_vrebuild, dim3((unsigned)((Bp + sh.vrows - 1) / sh.vrows)), dim3(1024), vsmem, st,
                           w, jwarm);
        LRS_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_svt_finish_state, dim3(1), dim3(1), 0, st, w);
        LRS_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_build_E, dim3((unsigned)((B + 15) / 16), (unsigned)((B + 15) / 16)), dim3(256), 0, st,
                           w, (int)B, tau);
        LRS_CHECK_LAUNCH();
    } else {
        // the tridiagonal stage's packed triangle (unless ga) + p vector; the products' staging; the fallback
        const size_t tsmem = sizeof(double) * ((sh.ga ? 0 : (size_t)Bp * (Bp + 1) / 2) + Bp);
        const size_t esmem = sizeof(double) * 2 * kEKc * eld(sh.nb);
        const size_t lds = std::max(std::max(tsmem, esmem), std::max(smem, vsmem));
        if (warm & LRS_SVT_MULTI_WG) {
            hipError_t ea = opt_in((const void *)k.tri, tsmem);
            if (ea == hipSuccess) ea = opt_in((const void *)k.cert, lds);
            if (ea != hipSuccess) return (int)ea;
            hipLaunchKernelGGL(k.tri, dim3(1), dim3(kEigThreads), tsmem, st, w);
            LRS_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_svt_eig_vals, dim3((unsigned)((4 * Bp + kEigMwThreads - 1) / kEigMwThreads)),
                               dim3(kEigMwThreads), 0, st, w);
            LRS_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_svt_eig_vecs, dim3((unsigned)((Bp + kEigMwThreads - 1) / kEigMwThreads)),
                               dim3(kEigMwThreads), 0, st, w);
            LRS_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_svt_eig_back, dim3((unsigned)((Bp + 15) / 16)), dim3(256), 0, st, w);
            LRS_CHECK_LAUNCH();
            hipLaunchKernelGGL(k.cert, dim3(1), dim3(kEigThreads), lds, st, w, (int)B, tau);
            LRS_CHECK_LAUNCH();
        } else {
            const hipError_t ea = opt_in((const void *)k.eig, lds);
            if (ea != hipSuccess) return (int)ea;
            hipLaunchKernelGGL(k.eig, dim3(1), dim3(kEigThreads), lds, st, w, (int)B, tau);
            LRS_CHECK_LAUNCH();
        }
    }
    if (s_out) {
        hipLaunchKernelGGL(k_sorted_singular_values, dim3(1), dim3(256), 0, st, w, (int)B, s_out);
        LRS_CHECK_LAUNCH();
    }
    return svt_apply(X, L2, c2, P, B, w, U, st);
}

extern "C" int lrs_svt_f32(const float *X, const float *L2, float c2, int64_t P, int64_t B, double tau, float *U,
                           double *s_out, int warm, void *ws, size_t ws_bytes, void *stream) {
    if (!U || tau < 0.0) return LRS_E_INVALID;
    int rc = lrs_svt_gram_f32(X, L2, c2, P, B, warm, ws, ws_bytes, stream);
    if (rc != LRS_OK) return rc;
    return lrs_svt_finish_f32(X, L2, c2, P, B, tau, U, s_out, warm, ws, ws_bytes, stream);
}

// Diagnostics (not in include/lrspnp.h): state words of the last call (host copy): V valid, V buffer,
// Jacobi rounds, sweeps, path (1 tridiagonal, 2 Jacobi fallback, 3 Jacobi, 4 wide tridiagonal, 5 its
// Jacobi fallback), Newton-Schulz steps and certificate flag of the wide tridiagonal chain, and word 7:
// 1 when LRS_SVT_WIDE_MW's reduction produced that chain's triangle; words 8-31 are spare.
extern "C" int lrs_diag_svt_state(void *ws, int64_t P, int64_t B, int *out32) {
    if (!ws || !out32 || P <= 0 || B <= 0) return LRS_E_INVALID;
    if (svt_shape_check(B, 0) != LRS_OK) return LRS_E_UNSUPPORTED;
    SvtWs w = svt_ws_layout(ws, B);
    return (int)hipMemcpy(out32, w.state, 32 * sizeof(int), hipMemcpyDeviceToHost);
}

// Diagnostics: the SVT apply alone (F = I - E from the last solve in ws): the kernel
// lrs_svt_finish_f32 launches for this band count (tools/time_svt_wide.py).
extern "C" int lrs_diag_svt_apply(const float *X, const float *L2, float c2, int64_t P, int64_t B, void *ws, float *U,
                                  void *stream) {
    if (!X || !U || !ws || P <= 0 || B <= 0) return LRS_E_INVALID;
    if (svt_shape_check(B, 0) != LRS_OK) return LRS_E_UNSUPPORTED;
    return svt_apply(X, L2, c2, P, B, svt_ws_layout(ws, B), U, (hipStream_t)stream);
}

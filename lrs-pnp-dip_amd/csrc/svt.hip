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
// Wide cubes (256 < B <= 512, svt_wide.h): 1 and 5 are tiled over column panels, and 2-4 run on the packed
// triangle in the workspace, or 3' over many workgroups with its certificate as GEMMs on the fp64 matrix cores
// (svt_wide_eig.h), its Householder reduction in one workgroup or one launch per column (svt_wide_mw.h).
//
// The stages: svt_gram.h (1, 2), svt_jacobi.h (3, 4), svt_eig.h (3'), svt_apply.h (5), svt_wide.h (the
// wide Gram), svt_wide_eig.h (the wide 3'), svt_wide_mw.h (its many-workgroup reduction); svt_ws.h has
// the workspace and the table of which form serves which band count.  Here: svt_plan (which chain a flag
// word asks for at a band count, decided once per call), one launcher per chain, and the C entry points.
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

// One call's chain, resolved once from (B, flags): the entry points read this and nothing else about the flag
// word.  Bp is B rounded up to even.
//   Bp > 512 (kWideMaxBp), or Bp > 256 (kMaxBp) with LRS_SVT_MULTI_WG: LRS_E_UNSUPPORTED.
//   Bp <= 256: LRS_SVT_WIDE_TRI and LRS_SVT_WIDE_MW are ignored.  LRS_SVT_JACOBI: the Jacobi chain; otherwise
//     LRS_SVT_MULTI_WG: the tridiagonal chain over many workgroups; otherwise that chain in one workgroup.
//   Bp > 256: LRS_SVT_WIDE_TRI without LRS_SVT_JACOBI: the wide tridiagonal chain, its Householder reduction over
//     many workgroups with LRS_SVT_WIDE_MW (mw_reduction); otherwise the wide Jacobi chain, LRS_SVT_WIDE_MW ignored.
//   warm: LRS_SVT_WARM.  warm_products (_gram forms A0 = V^T G V): warm, on a Jacobi chain, narrow or wide.
//   reset_state (_gram zeroes the state words): the flag word is zero once the ignored bits are dropped, or the
//     chain is the wide tridiagonal one and LRS_SVT_WARM is clear.  So a cold LRS_SVT_JACOBI or LRS_SVT_MULTI_WG
//     call at Bp <= 256 keeps the words of the call before it, which is harmless: k_jacobi_lds ignores V when
//     its warm argument is 0, and the tridiagonal chains rewrite words 0, 1 and 4.
enum SvtChain { kSvtTri = 0, kSvtTriMw = 1, kSvtJacobi = 2, kSvtWideJacobi = 3, kSvtWideTri = 4 };
struct SvtPlan {
    int rc, warm;   // rc: LRS_OK or LRS_E_UNSUPPORTED (the other fields are then unset)
    SvtChain chain;
    bool mw_reduction, reset_state, warm_products;
};

static SvtPlan svt_plan(int64_t B, int flags) {
    SvtPlan p{};
    const int64_t Bp = B + (B & 1);
    const bool wide = Bp > kMaxBp, jacobi = flags & LRS_SVT_JACOBI;
    p.rc = Bp > kWideMaxBp || (wide && (flags & LRS_SVT_MULTI_WG)) ? LRS_E_UNSUPPORTED : LRS_OK;
    if (p.rc != LRS_OK) return p;
    p.chain = wide ? ((flags & LRS_SVT_WIDE_TRI) && !jacobi ? kSvtWideTri : kSvtWideJacobi)
                   : jacobi ? kSvtJacobi : (flags & LRS_SVT_MULTI_WG) ? kSvtTriMw : kSvtTri;
    const bool wide_tri = p.chain == kSvtWideTri;
    p.warm = flags & LRS_SVT_WARM;
    p.mw_reduction = wide_tri && (flags & LRS_SVT_WIDE_MW);
    p.warm_products = p.warm && (p.chain == kSvtJacobi || p.chain == kSvtWideJacobi);
    p.reset_state = wide_tri ? !p.warm : !(flags & ~(LRS_SVT_WIDE_TRI | LRS_SVT_WIDE_MW));
    return p;
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
    const SvtPlan plan = svt_plan(B, warm);
    if (plan.rc != LRS_OK) return plan.rc;
    if (ws_bytes < svt_ws_offsets(B).total) return LRS_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    SvtWs w = svt_ws_layout(ws, B);
    if (plan.reset_state) {
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
    if (plan.warm_products) {
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

// Stage 2's launchers, one per chain.  What they share: the workspace, this band count's forms, and the LDS of
// the Jacobi solve (smem) and the V replay (vsmem), of the tridiagonal stage (tsmem: the packed triangle unless
// ga, + p vector) and the most a phase of the narrow tridiagonal chains needs (lds: the products' staging too).
struct SvtSolve {
    SvtWs w;
    int B, Bp;
    double tau;
    SvtShape sh;
    SvtKernels k;
    size_t smem, vsmem, tsmem, lds;
    hipStream_t st;
};
// one launch on the call's stream, the workspace first among the kernel's arguments, and its check
#define SVT_LAUNCH(c, kernel, grid, block, lds, ...)                                \
    do {                                                                            \
        hipLaunchKernelGGL(kernel, grid, block, lds, (c).st, (c).w, ##__VA_ARGS__); \
        LRS_CHECK_LAUNCH();                                                         \
    } while (0)

// dynamic LDS above 64 KiB must be opted into; request exactly what this shape needs
static const auto opt_in = [](const void *kernel, size_t bytes) {
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
};

// eigenvalues, inverse iteration and back-transformation of a tridiagonal chain over many workgroups
static int svt_vals_vecs_back(const SvtSolve &c, TriKernel vals, TriKernel vecs, TriKernel back) {
    SVT_LAUNCH(c, vals, dim3((unsigned)((4 * c.Bp + kEigMwThreads - 1) / kEigMwThreads)), dim3(kEigMwThreads), 0);
    SVT_LAUNCH(c, vecs, dim3((unsigned)((c.Bp + kEigMwThreads - 1) / kEigMwThreads)), dim3(kEigMwThreads), 0);
    SVT_LAUNCH(c, back, dim3((unsigned)((c.Bp + 15) / 16)), dim3(256), 0);
    return LRS_OK;
}

// E, and F = I - E in w.Fp, after a chain that does not write them itself
static int svt_build_E(const SvtSolve &c) {
    SVT_LAUNCH(c, k_build_E, dim3((unsigned)((c.B + 15) / 16), (unsigned)((c.B + 15) / 16)), dim3(256), 0, c.B, c.tau);
    return LRS_OK;
}

static int svt_run_tri(const SvtSolve &c) {
    const hipError_t ea = opt_in((const void *)c.k.eig, c.lds);
    if (ea != hipSuccess) return (int)ea;
    SVT_LAUNCH(c, c.k.eig, dim3(1), dim3(kEigThreads), c.lds, c.B, c.tau);
    return LRS_OK;
}

// the phases of k_svt_eig as five kernels, three of them over many workgroups
static int svt_run_tri_mw(const SvtSolve &c) {
    hipError_t ea = opt_in((const void *)c.k.tri, c.tsmem);
    if (ea == hipSuccess) ea = opt_in((const void *)c.k.cert, c.lds);
    if (ea != hipSuccess) return (int)ea;
    SVT_LAUNCH(c, c.k.tri, dim3(1), dim3(kEigThreads), c.tsmem);
    const int rc = svt_vals_vecs_back(c, k_svt_eig_vals, k_svt_eig_vecs, k_svt_eig_back);
    if (rc != LRS_OK) return rc;
    SVT_LAUNCH(c, c.k.cert, dim3(1), dim3(kEigThreads), c.lds, c.B, c.tau);
    return LRS_OK;
}

// narrow and wide alike: the shape class picks k_jacobi_lds<ga> and the replay's rows
static int svt_run_jacobi(const SvtSolve &c, int jwarm) {
    hipError_t ea = opt_in((const void *)c.k.jacobi, c.smem);
    if (ea == hipSuccess) ea = opt_in((const void *)k_jacobi_vrebuild, c.vsmem);
    if (ea != hipSuccess) return (int)ea;
    SVT_LAUNCH(c, c.k.jacobi, dim3(1), dim3(kJacobiThreads), c.smem, jwarm);
    const dim3 vgrid((unsigned)((c.Bp + c.sh.vrows - 1) / c.sh.vrows));
    SVT_LAUNCH(c, k_jacobi_vrebuild, vgrid, dim3(1024), c.vsmem, jwarm);
    SVT_LAUNCH(c, k_svt_finish_state, dim3(1), dim3(1), 0);
    return svt_build_E(c);
}

// tridiagonalisation, eigenvalues, inverse iteration, back-transformation; S = V^T V and its
// certificate, kWtMaxNs gated Newton-Schulz steps, the gated Jacobi fallback; then E
static int svt_run_wide_tri(const SvtSolve &c, bool mw_reduction) {
    const int Bp = c.Bp;
    const hipError_t ea = opt_in((const void *)k_svt_eig_wide_fb_vrebuild, c.vsmem);
    if (ea != hipSuccess) return (int)ea;
    if (mw_reduction) {
        // the reduction over many workgroups: launch k forms reflector k + 1 and applies reflector k
        for (int kc = -1; kc <= Bp - 2; ++kc)
            SVT_LAUNCH(c, k_svt_eig_wide_mw, dim3((unsigned)mw_nwg(Bp, kc)), dim3(kMwThreads), 0, kc);
    } else {
        SVT_LAUNCH(c, k_svt_eig_wide_tri, dim3(1), dim3(kEigThreads), sizeof(double) * Bp);
    }
    const int rc = svt_vals_vecs_back(c, k_svt_eig_wide_vals, k_svt_eig_wide_vecs, k_svt_eig_wide_back);
    if (rc != LRS_OK) return rc;
    const dim3 g64((unsigned)((Bp + 63) / 64), (unsigned)((Bp + 63) / 64));
    for (int step = 0; step <= kWtMaxNs; ++step) {
        if (step > 0) SVT_LAUNCH(c, k_svt_eig_wide_gemm<true>, g64, dim3(256), 0, step);
        SVT_LAUNCH(c, k_svt_eig_wide_gemm<false>, g64, dim3(256), 0, step);
        SVT_LAUNCH(c, k_svt_eig_wide_cert, dim3(1), dim3(kEigThreads), 0, step);
    }
    SVT_LAUNCH(c, k_svt_eig_wide_fb_jacobi, dim3(1), dim3(kJacobiThreads), c.smem);
    const dim3 vgrid((unsigned)((Bp + c.sh.vrows - 1) / c.sh.vrows));
    SVT_LAUNCH(c, k_svt_eig_wide_fb_vrebuild, vgrid, dim3(1024), c.vsmem);
    SVT_LAUNCH(c, k_svt_eig_wide_fb_state, dim3(1), dim3(1), 0);
    return svt_build_E(c);
}

// Stage 2: the plan's eigen chain (runs beside the sparse-coding kernel), E, U.
extern "C" int lrs_svt_finish_f32(const float *X, const float *L2, float c2, int64_t P, int64_t B, double tau,
                                  float *U, double *s_out, int warm, void *ws, size_t ws_bytes, void *stream) {
    if (!X || !U || !ws || P <= 0 || B <= 0 || tau < 0.0) return LRS_E_INVALID;
    const SvtPlan plan = svt_plan(B, warm);
    if (plan.rc != LRS_OK) return plan.rc;
    if (ws_bytes < svt_ws_offsets(B).total) return LRS_E_WORKSPACE;
    const SvtShape sh = svt_shape(B);
    const int Bp = (int)(B + (B & 1));
    const size_t smem = jacobi_lds(Bp, sh.ga), vsmem = vrebuild_lds(Bp);
    const size_t tsmem = sizeof(double) * ((sh.ga ? 0 : (size_t)Bp * (Bp + 1) / 2) + Bp);
    const size_t lds = std::max(std::max(tsmem, sizeof(double) * 2 * kEKc * eld(sh.nb)), std::max(smem, vsmem));
    const SvtSolve c{svt_ws_layout(ws, B), (int)B, Bp, tau, sh, svt_kernels(sh), smem, vsmem, tsmem, lds,
                     (hipStream_t)stream};
    int rc = LRS_OK;
    switch (plan.chain) {
    case kSvtTri: rc = svt_run_tri(c); break;
    case kSvtTriMw: rc = svt_run_tri_mw(c); break;
    case kSvtJacobi:
    case kSvtWideJacobi: rc = svt_run_jacobi(c, plan.warm); break;
    case kSvtWideTri: rc = svt_run_wide_tri(c, plan.mw_reduction); break;
    }
    if (rc != LRS_OK) return rc;
    if (s_out) SVT_LAUNCH(c, k_sorted_singular_values, dim3(1), dim3(256), 0, c.B, s_out);
    return svt_apply(X, L2, c2, P, B, c.w, U, c.st);
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
    if (svt_plan(B, 0).rc != LRS_OK) return LRS_E_UNSUPPORTED;
    SvtWs w = svt_ws_layout(ws, B);
    return (int)hipMemcpy(out32, w.state, 32 * sizeof(int), hipMemcpyDeviceToHost);
}

// Diagnostics (host only, no device touched): the plan of (B, flags) as chain (SvtChain), warm,
// mw_reduction, reset_state, warm_products; words 5-7 are spare.  Returns the plan's return code.
extern "C" int lrs_diag_svt_plan(int64_t B, int flags, int *out8) {
    if (B <= 0 || !out8) return LRS_E_INVALID;
    const SvtPlan p = svt_plan(B, flags);
    const int words[8] = {p.chain, p.warm, p.mw_reduction, p.reset_state, p.warm_products, 0, 0, 0};
    std::copy(words, words + 8, out8);
    return p.rc;
}

// Diagnostics: the SVT apply alone (F = I - E from the last solve in ws): the kernel
// lrs_svt_finish_f32 launches for this band count (tools/time_svt_wide.py).
extern "C" int lrs_diag_svt_apply(const float *X, const float *L2, float c2, int64_t P, int64_t B, void *ws, float *U,
                                  void *stream) {
    if (!X || !U || !ws || P <= 0 || B <= 0) return LRS_E_INVALID;
    if (svt_plan(B, 0).rc != LRS_OK) return LRS_E_UNSUPPORTED;
    return svt_apply(X, L2, c2, P, B, svt_ws_layout(ws, B), U, (hipStream_t)stream);
}

// The sparse-coding paths behind lrs_ista_f32 / lrs_ista_pat_f32: the one declaration of every
// function the ISTA translation units call across files, and the host helpers they share.  Every
// definer includes this header, so a signature that drifts fails to compile instead of linking.
#pragma once
#include <type_traits>

#include "lrs_common.h"

namespace lrs {

// 16-atom tiles the row-split and per-pattern kernels are instantiated for (K <= 512)
inline int ista_nq(int64_t K) { return K <= 64 ? 4 : K <= 128 ? 8 : K <= 256 ? 16 : 32; }

// f(std::integral_constant<int, NQ>, std::bool_constant<accel>) for the instantiated NQ = ista_nq(K):
// a launcher writes its NQ -> kernel table once, as a generic lambda
template <class F>
inline int ista_dispatch_nq(int NQ, bool accel, F &&f) {
    auto with = [&](auto nq) { return accel ? f(nq, std::true_type{}) : f(nq, std::false_type{}); };
    switch (NQ) {
    case 4: return with(std::integral_constant<int, 4>{});
    case 8: return with(std::integral_constant<int, 8>{});
    case 16: return with(std::integral_constant<int, 16>{});
    default: return with(std::integral_constant<int, 32>{});
    }
}

// The dictionary images at the head of a workspace, in MFMA fragment order (ista_rs.hip):
//   DAf [NT][NQ][64] float4, DTf the same, then on the per-pattern path (npat > 0) QAf [npat][NQ][NQ][64].
// n_pad sets the images' row count (the kernels index them with NT = n_pad / 16): a workspace sized
// from n covers n_pad = round_up(n, 16); a larger n_pad needs its own size.
struct IstaImages {
    int64_t NT, NQ, npat;
    IstaImages(int64_t n_pad, int64_t K, int64_t npat = 0) : NT(round_up(n_pad, 16) / 16), NQ(ista_nq(K)), npat(npat) {}
    int64_t d_float4() const { return NT * NQ * 64; }   // one of DAf / DTf
    size_t bytes() const { return (size_t)(2 * d_float4() + npat * NQ * NQ * 64) * sizeof(float4); }
    float4 *DAf(void *ws) const { return reinterpret_cast<float4 *>(ws); }
    float4 *DTf(void *ws) const { return DAf(ws) + d_float4(); }
    float4 *QAf(void *ws) const { return DTf(ws) + d_float4(); }
    // The size limits of the kernels that read the images, and the workspace: K <= 512 atoms, 32-bit buffer
    // offsets (t * NQ + q) * 1024 into an image, and on the per-pattern path n and npat within the plan's
    // packing.  workspace_first: which of the two a call that misses both reports.  lrs_ista_f32 has always
    // reported the limit, the per-pattern entries the workspace; K comes first in both.
    int check(int64_t n, int64_t K, const void *ws, size_t ws_bytes, bool workspace_first) const {
        if (K < 1 || K > 512) return LRS_E_UNSUPPORTED;
        const bool fits = ws && ws_bytes >= bytes();
        if (workspace_first && !fits) return LRS_E_WORKSPACE;
        if (NT * NQ * 1024 >= ((int64_t)1 << 31)) return LRS_E_UNSUPPORTED;
        if (npat > 0 && (n > INT32_MAX / 2 || npat > 65535)) return LRS_E_UNSUPPORTED;
        return fits ? LRS_OK : LRS_E_WORKSPACE;
    }
};

// The argument checks lrs_ista_f32 and lrs_ista_pat_f32 share.  Each entry adds its own: the
// pointers, the bound on nb, and the lrs_ista_opts.algorithm values it accepts.
inline int ista_check_args(int64_t n, int64_t n_pad, int64_t K, int64_t nb, int Nit, int prox,
                           const lrs_ista_opts *opts) {
    if (n <= 0 || nb < 0 || Nit < 0 || K <= 0) return LRS_E_INVALID;
    if (n_pad % 16 != 0 || n_pad < n || n_pad > (int64_t)1 << 20) return LRS_E_INVALID;
    if (prox != LRS_PROX_NLM && prox != LRS_PROX_SOFT && prox != LRS_PROX_NLM_MATLAB) return LRS_E_INVALID;
    if (!opts) return LRS_OK;
    if (opts->precision != LRS_ISTA_F32 && opts->precision != LRS_ISTA_SPLIT_BF16) return LRS_E_INVALID;
    if (opts->max_workgroups < 0) return LRS_E_INVALID;
    if (opts->warm_start != 0 && opts->warm_start != 1) return LRS_E_INVALID;
    if (opts->accel != LRS_ISTA_ACCEL_NONE && opts->accel != LRS_ISTA_ACCEL_FISTA) return LRS_E_INVALID;
    return LRS_OK;
}

// ---- ista_rs.hip: the row-split kernel (any n, K <= 512, every prox) ---------------------------
size_t ista_rs_workspace(int64_t n, int64_t K);
// the two fragment-ordered dictionary images (also read by the per-pattern Gram kernel)
int ista_rs_images(const float *D, int64_t n, int64_t K, const IstaImages &im, void *ws, hipStream_t st);
int ista_rs_launch(const float *Yb, const uint8_t *obs, const float *D, int64_t n, int64_t n_pad, int64_t K, int64_t nb,
                   const float *alpha, const double *thr, int Nit, int prox, float *coefs, float *phi, void *ws,
                   size_t ws_bytes, int64_t max_wg, hipStream_t st, const float *x0, bool accel);
// NLmeansfilter(g, 3, 3, h) of nvec columns of length K (the MATLAB-variant prox)
int nlm_matlab_col_launch(const float *g, int64_t ldg, float *out, int64_t ldo, int64_t K, int64_t nvec, double h,
                          const double *h_per_vec, hipStream_t st);

// ---- ista_generic.hip: the dense-GEMM path (any K; the only one for K > 512) -------------------
// accel: one more chunk of coefficients (x_{k-1}) behind the plain layout
size_t ista_generic_workspace(int64_t n, int64_t K, bool accel);
int ista_generic(const float *Yb, const uint8_t *obs, const float *D, int64_t n, int64_t n_pad, int64_t K, int64_t nb,
                 const float *alpha, const double *thr, int Nit, int prox, float *coefs, float *phi, void *ws,
                 size_t ws_bytes, hipStream_t st, bool accel);

// ---- dipnet.hip: C = op(A) op(B), fp32-accurate, split-K partials in `part` --------------------
int64_t dense_gemm_part_floats(int M, int N, int K);
int dense_gemm(int TA, int TB, const float *A, const float *B, float *C, int M, int N, int K, float *part,
               int64_t part_cap, hipStream_t st);

}  // namespace lrs

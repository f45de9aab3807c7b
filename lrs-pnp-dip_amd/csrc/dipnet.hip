// DIP low-rank prox: C-ABI of the layer primitives and the sequential-network training engine.
//
// Reference: main_LRS_PnP_DIP_1-LiP.py:208-264 (get_DIP_out: fresh my_Lipschitz_Unet, Adam,
// masked MSE, early stopping) and models/my_Lipschitz_Unet.py:21-148.  The engine launches one
// training step as ~8 kernels per conv unit from C++ (no per-layer Python), and can capture the
// step in a hipGraph and replay it: the Adam step count and the early-stopping state live in
// device memory, so a replayed step is exactly the eager step.
// dip_launch.h: geometry and the kernel launchers; dipnet_plan.h: the net, its layout and plan.
// Every node with a conv product (CONV, and the Deep Decoder's DECODE) runs one path: product -> the
// stage tail the plan names (DECODE: [bilinear x2 +] activation) -> BatchNorm; a node's generic
// BatchNorm call is lrs_dipnet::node_bn_fwd / node_bn_bwd, a bias that may be absent bias_in.
#include "dipnet_plan.h"

// Dense fp32-accurate GEMM for the library's other components (the K > 512 ISTA path,
// ista_generic.hip; declared in ista_paths.h):
// C[M][N] = op(A) op(B) with the DIP engine's split-bf16 / f32 kernels, split-K summed in fixed
// order (deterministic).  part: >= dense_gemm_part_floats(M, N, K) floats.
namespace lrs {
int64_t dense_gemm_part_floats(int M, int N, int K) { return gemm_part_floats(M, N, K); }
int dense_gemm(int TA, int TB, const float *A, const float *B, float *C, int M, int N, int K, float *part,
               int64_t part_cap, hipStream_t st) {
    return gemm(LRS_DIP_SPLIT_BF16, TA, TB, A, B, C, nullptr, nullptr, M, N, K, part, part_cap, st);
}
}  // namespace lrs

// ============================================================================================
// Primitive C ABI
// ============================================================================================
extern "C" int lrs_conv2d_out_size(int H, int W, int k, int stride, int pad, int upsample, int *Ho, int *Wo) {
    ConvGeom g;
    const int rc = make_geom(1, H, W, k, stride, pad, LRS_PAD_ZERO, upsample, g);
    if (rc) return rc;
    if (Ho) *Ho = g.Ho; if (Wo) *Wo = g.Wo;
    return LRS_OK;
}

extern "C" int64_t lrs_conv2d_col_size(int Cin, int H, int W, int k, int stride, int pad, int upsample) {
    ConvGeom g;
    if (make_geom(Cin, H, W, k, stride, pad, LRS_PAD_ZERO, upsample, g)) return -1;
    return plain_unit(g) ? 0 : (int64_t)Cin * k * k * g.Ho * g.Wo;
}

// conv workspace: [dcol: Kc*P floats when not plain][split-K partials][weight planes (bf16)]
struct ConvWs {
    int64_t dcol, part, wpre_floats;
};
inline ConvWs conv_ws(const ConvGeom &g, int Cout) {
    ConvWs w;
    w.dcol = plain_unit(g) ? 0 : (int64_t)g.Cin * g.k * g.k * g.Ho * g.Wo;
    w.part = conv_part_floats(g, Cout);
    w.wpre_floats = (plain_unit(g) && !pw_ok(g, Cout)) ? 0 : (wprep_elems(g, Cout, false).total() + 7) / 2;
    return w;
}

extern "C" size_t lrs_conv2d_workspace(int Cin, int H, int W, int Cout, int k, int stride, int pad, int upsample,
                                       const lrs_dip_opts *opts) {
    ConvGeom g;
    if (make_geom(Cin, H, W, k, stride, pad, LRS_PAD_ZERO, upsample, g, opts) || Cout <= 0) return 0;
    const ConvWs w = conv_ws(g, Cout);
    return (size_t)(w.dcol + w.part + w.wpre_floats) * sizeof(float) + 256;
}

extern "C" int lrs_conv2d_fwd_f32(const float *x, int Cin, int H, int W, const float *w, const float *bias, int Cout,
                                  int k, int stride, int pad, int pad_mode, int upsample, float *col, float *y,
                                  const lrs_dip_opts *opts, void *ws, size_t ws_bytes, void *stream) {
    ConvGeom g;
    int rc = make_geom(Cin, H, W, k, stride, pad, pad_mode, upsample, g, opts);
    if (rc) return rc;
    if (!x || !w || !y || Cout <= 0) return LRS_E_INVALID;
    // col == NULL: implicit GEMM, or for a 1x1 conv the pointwise kernel on pre-split weights
    const bool implicit = !col && (!plain_unit(g) || pw_ok(g, Cout));
    if (implicit && !plain_unit(g) && !conv_implicit_ok(g, Cout)) return LRS_E_UNSUPPORTED;
    const ConvWs cw = conv_ws(g, Cout);
    const int64_t need = implicit ? cw.dcol + cw.part + cw.wpre_floats : cw.part;
    if (need > 0 && (!ws || ws_bytes < (size_t)need * sizeof(float))) return LRS_E_WORKSPACE;
    float *pt = implicit ? (float *)ws + cw.dcol : (float *)ws;
    __bf16 *wp = implicit ? (__bf16 *)((float *)ws + cw.dcol + cw.part) : nullptr;
    if (implicit && (rc = wprep(g, w, Cout, wp, nullptr, (hipStream_t)stream))) return rc;
    return conv_fwd(g, x, w, bias, Cout, col, y, pt, cw.part, (hipStream_t)stream, wp);
}

extern "C" int lrs_conv2d_bwd_f32(const float *gy, const float *col, const float *w, const float *w_div, int Cin,
                                  int H, int W, int Cout, int k, int stride, int pad, int pad_mode, int upsample,
                                  float *gx, float *gw, const lrs_dip_opts *opts, void *ws, size_t ws_bytes,
                                  void *stream) {
    ConvGeom g;
    int rc = make_geom(Cin, H, W, k, stride, pad, pad_mode, upsample, g, opts);
    if (rc) return rc;
    if (!gy || !col || !w || !gw || Cout <= 0) return LRS_E_INVALID;
    const ConvWs cw = conv_ws(g, Cout);
    if (ws_bytes < (size_t)(cw.part + cw.dcol) * sizeof(float) || (!ws && cw.part + cw.dcol > 0))
        return LRS_E_WORKSPACE;
    float *dc = cw.dcol ? (float *)ws : nullptr;
    float *pt = (float *)ws + cw.dcol;
    rc = conv_wgrad(g, gy, col, w_div, Cout, gw, pt, cw.part, (hipStream_t)stream, false);
    if (rc || !gx) return rc;
    return conv_dgrad(g, gy, w, Cout, gx, dc, pt, cw.part, (hipStream_t)stream, 0, false, nullptr);
}

extern "C" int lrs_conv2d_bwd_x_f32(const float *gy, const float *x, const float *w, const float *w_div, int Cin,
                                    int H, int W, int Cout, int k, int stride, int pad, int pad_mode, int upsample,
                                    float *gx, float *gw, const lrs_dip_opts *opts, void *ws, size_t ws_bytes,
                                    void *stream) {
    ConvGeom g;
    int rc = make_geom(Cin, H, W, k, stride, pad, pad_mode, upsample, g, opts);
    if (rc) return rc;
    if (!gy || !x || !w || !gw || Cout <= 0) return LRS_E_INVALID;
    if (!conv_implicit_ok(g, Cout)) return LRS_E_UNSUPPORTED;
    const ConvWs cw = conv_ws(g, Cout);
    const int64_t need = cw.dcol + cw.part + cw.wpre_floats;
    if (ws_bytes < (size_t)need * sizeof(float) || (!ws && need > 0)) return LRS_E_WORKSPACE;
    float *dc = cw.dcol ? (float *)ws : nullptr;
    float *pt = (float *)ws + cw.dcol;
    __bf16 *wp = cw.wpre_floats ? (__bf16 *)((float *)ws + cw.dcol + cw.part) : nullptr;
    if (wp && gx && (rc = wprep(g, w, Cout, wp, wp + wprep_elems(g, Cout, false).fwd, (hipStream_t)stream))) return rc;
    rc = conv_wgrad(g, gy, x, w_div, Cout, gw, pt, cw.part, (hipStream_t)stream, true);
    if (rc || !gx) return rc;
    return conv_dgrad(g, gy, w, Cout, gx, dc, pt, cw.part, (hipStream_t)stream, 0, true, wp);
}

extern "C" size_t lrs_bn_act_workspace(int C, int64_t P) {
    if (C <= 0 || P <= 0) return 0;
    return (size_t)bn_part_doubles(C, P) * sizeof(double) + 256;
}

static int bn_ws(void *ws, size_t ws_bytes, int C, int64_t P, double **part) {
    if (!ws || ws_bytes < lrs_bn_act_workspace(C, P)) return LRS_E_WORKSPACE;
    *part = (double *)ws;
    return LRS_OK;
}

extern "C" int lrs_bn_act_fwd_f32(const float *z, float *y, const float *gamma, const float *beta, float *mean,
                                  float *invstd, float *run_mean, float *run_var, int C, int64_t P, int act,
                                  float eps, float momentum, void *ws, size_t ws_bytes, void *stream) {
    if (!z || !y || C <= 0 || P <= 0 || P > INT32_MAX) return LRS_E_INVALID;
    if (gamma && (!beta || !mean || !invstd)) return LRS_E_INVALID;
    double *part;
    const int rc = bn_ws(ws, ws_bytes, C, P, &part);
    if (rc) return rc;
    return bn_fwd(z, y, gamma, beta, mean, invstd, run_mean, run_var, C, P, act, eps, momentum, part,
                  (hipStream_t)stream);
}

extern "C" int lrs_bn_act_bwd_f32(const float *gy, const float *y, const float *z, const float *gamma,
                                  const float *mean, const float *invstd, float *gz, float *ggamma, float *gbeta,
                                  float *gbias, int C, int64_t P, int act, void *ws, size_t ws_bytes, void *stream) {
    if (!gy || !y || !gz || C <= 0 || P <= 0 || P > INT32_MAX) return LRS_E_INVALID;
    if (gamma && (!z || !mean || !invstd || !ggamma || !gbeta)) return LRS_E_INVALID;
    double *part;
    const int rc = bn_ws(ws, ws_bytes, C, P, &part);
    if (rc) return rc;
    return bn_bwd(gy, y, z, gamma, mean, invstd, gz, ggamma, gbeta, gbias, C, P, act, part, (hipStream_t)stream);
}

// The engine's one-launch small-map conv + BatchNorm (k_conv_bn_dir, dip_dir.h) on its own: the same
// launch dipnet_forward makes for a conv with BN on a map of <= kDirMaxP pixels.
extern "C" int lrs_conv_bn_small_f32(const float *x, int Cin, int H, int W, const float *w, const float *bias, int Cout,
                                     int k, int stride, int pad, int pad_mode, int upsample, const float *gamma,
                                     const float *beta, int lip, int act, float *z, float *y, float *mean, float *invstd,
                                     float *run_mean, float *run_var, void *stream) {
    ConvGeom g;
    int rc = make_geom(Cin, H, W, k, stride, pad, pad_mode, upsample, g);
    if (rc) return rc;
    if (!x || !w || !gamma || !beta || !z || !y || !mean || !invstd || Cout <= 0 || Cout > 65535 ||
        (!run_mean) != (!run_var) || (lip != 0 && lip != 1))
        return LRS_E_INVALID;
    if (act != LRS_ACT_NONE && act != LRS_ACT_LRELU && act != LRS_ACT_SIGMOID) return LRS_E_INVALID;
    DirGeom dg;
    if (!dir_geom(g, dg)) return LRS_E_UNSUPPORTED;
    const int P = g.Ho * g.Wo;
    const BnArgs a{z, y, gamma, beta, mean, invstd, run_mean, run_var, nullptr, Cout, P, 1, P, 1, act, kBnEps, kBnMomentum, lip, 0};
    dir_launch(g, dg, x, w, bias, a, (hipStream_t)stream);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// The Deep Decoder stage's two kernels (dip_up.h) on their own
extern "C" int lrs_up2_bilinear_act_fwd_f32(const float *x, int C, int H, int W, int act, float *y, void *stream) {
    if (!x || !y || !dec_act_ok(act)) return LRS_E_INVALID;
    return up2_fwd(x, C, H, W, act, y, (hipStream_t)stream);
}

extern "C" int lrs_up2_bilinear_act_bwd_f32(const float *gy, const float *y, int C, int H, int W, int act, float *gx,
                                            void *stream) {
    if (!gy || !y || !gx || !dec_act_ok(act)) return LRS_E_INVALID;
    return up2_bwd(gy, y, C, H, W, act, gx, (hipStream_t)stream);
}

extern "C" size_t lrs_sigma_max_workspace(int n) {
    if (n <= 0) return 0;
    return (size_t)n * kSnGramDoubles * sizeof(double) + (size_t)n * sizeof(SnConv) + 256;
}

extern "C" int lrs_sigma_max_f32(const float *const *W, float *const *Wn, const int *rows, const int *cols, int n,
                                 float ln_lambda, float *sigma, float *scale, void *ws, size_t ws_bytes,
                                 void *stream) {
    if (n <= 0) return LRS_OK;
    if (!W || !rows || !cols || !sigma || !scale || !(ln_lambda > 0.0f)) return LRS_E_INVALID;
    if (!ws || ws_bytes < lrs_sigma_max_workspace(n)) return LRS_E_WORKSPACE;
    std::vector<SnConv> tab(n);
    int64_t maxe = 0;
    for (int i = 0; i < n; ++i) {
        if (!W[i] || rows[i] <= 0 || cols[i] <= 0) return LRS_E_INVALID;
        if ((rows[i] < cols[i] ? rows[i] : cols[i]) > kSnMaxDim) return LRS_E_UNSUPPORTED;
        tab[i] = SnConv{W[i], Wn ? Wn[i] : nullptr, rows[i], cols[i]};
        const int64_t e = (int64_t)rows[i] * cols[i];
        if (e > maxe) maxe = e;
    }
    double *gram = (double *)ws;
    SnConv *tdev = (SnConv *)((char *)ws + (size_t)n * kSnGramDoubles * sizeof(double));
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(tdev, tab.data(), sizeof(SnConv) * n, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return (int)e;
    e = hipStreamSynchronize(st);   // the host table is a local
    if (e != hipSuccess) return (int)e;
    return sn_launch(tdev, n, maxe, gram, sigma, scale, ln_lambda, Wn != nullptr, st);
}

// diagnostics: phase timestamps (wall_clock64 ticks) of the sigma kernel, 8 int64 per matrix:
// [start, Gram loaded, Lanczos done, multisection done, Lanczos steps]
extern "C" int lrs_diag_sigma_phases(const float *const *W, const int *rows, const int *cols, int n, void *ws,
                                     size_t ws_bytes, long long *prof, void *stream) {
    if (n <= 0 || !W || !prof) return LRS_E_INVALID;
    if (!ws || ws_bytes < lrs_sigma_max_workspace(n) + 2 * n * sizeof(float)) return LRS_E_WORKSPACE;
    std::vector<SnConv> tab(n);
    for (int i = 0; i < n; ++i) tab[i] = SnConv{W[i], nullptr, rows[i], cols[i]};
    double *gram = (double *)ws;
    SnConv *tdev = (SnConv *)((char *)ws + (size_t)n * kSnGramDoubles * sizeof(double));
    float *sig = (float *)((char *)ws + lrs_sigma_max_workspace(n));
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(tdev, tab.data(), sizeof(SnConv) * n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return (int)e;
    return sn_launch(tdev, n, 0, gram, sig, sig + n, 1.0f, false, st, prof);
}

extern "C" int lrs_adam_f32(float *p, const float *g, float *m, float *v, int64_t n, const int *step, float lr,
                            float beta1, float beta2, float eps, void *stream) {
    if (!p || !g || !m || !v || !step || n < 0) return LRS_E_INVALID;
    if (n == 0) return LRS_OK;
    hipLaunchKernelGGL(k_adam, dim3(ew_blocks((n + 3) / 4, 8192)), dim3(kEw), 0, (hipStream_t)stream, p, g, m, v, n, step, lr,
                       beta1, beta2, eps, AdamPend{});
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// The mask's channel count (1: [P], broadcast over the channels; C: per element [C][P]) -> its row
// stride in floats (0 / P; 0 without a mask); -1 for any other count.
static int64_t mask_stride(const float *mask, int mask_channels, int C, int64_t P) {
    if (mask_channels != 1 && mask_channels != C) return -1;
    return (mask && mask_channels == C && C > 1) ? P : 0;
}

// float4 mask loads: row c starts at mask + c * mstride, 16-B aligned for every c when the base is
// and the stride is a multiple of 4 floats (0, or P with P % 4 == 0)
static bool mask_al16(const float *mask, int64_t mstride) { return !mask || (al16(mask) && mstride % 4 == 0); }

// n_mean: the element count of the mean (C P, or fewer for a framed output: k_masked_mse_n)
static int masked_mse(const float *out, const float *target, const float *mask, int mask_channels, int C, int64_t P,
                      int64_t n_mean, float *gout, double *loss_acc, void *stream) {
    if (!out || !target || !loss_acc || C <= 0 || P <= 0 || n_mean <= 0 || n_mean > (int64_t)C * P) return LRS_E_INVALID;
    const int64_t mstride = mask_stride(mask, mask_channels, C, P);
    if (mstride < 0) return LRS_E_INVALID;
    const int vec = (P % 4 == 0 && al16(out) && al16(target) && mask_al16(mask, mstride) && (!gout || al16(gout))) ? 1 : 0;
    int64_t S = (512 + C - 1) / C;   // ~512 workgroups over the C channels (fewer loss atomics)
    S = std::max<int64_t>(1, std::min<int64_t>(S, (P + 1023) / 1024));
    int64_t chunk = (P + S - 1) / S;
    if (vec) chunk = (chunk + 3) & ~(int64_t)3;
    if (chunk > INT32_MAX || C > 65535) return LRS_E_UNSUPPORTED;
    if (n_mean == (int64_t)C * P)
        hipLaunchKernelGGL(k_masked_mse, dim3((unsigned)S, (unsigned)C), dim3(256), 0, (hipStream_t)stream, out, target,
                           mask, mstride, C, P, (int)chunk, vec, gout, loss_acc);
    else
        hipLaunchKernelGGL(k_masked_mse_n, dim3((unsigned)S, (unsigned)C), dim3(256), 0, (hipStream_t)stream, out, target,
                           mask, mstride, n_mean, P, (int)chunk, vec, gout, loss_acc);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

extern "C" int lrs_masked_mse_cmask_f32(const float *out, const float *target, const float *mask, int mask_channels,
                                        int C, int64_t P, float *gout, double *loss_acc, void *stream) {
    return masked_mse(out, target, mask, mask_channels, C, P, (int64_t)C * P, gout, loss_acc, stream);
}

extern "C" int lrs_masked_mse_framed_f32(const float *out, const float *target, const float *mask, int mask_channels,
                                         int C, int64_t P, int64_t n_mean, float *gout, double *loss_acc,
                                         void *stream) {
    return masked_mse(out, target, mask, mask_channels, C, P, n_mean, gout, loss_acc, stream);
}

extern "C" int lrs_masked_mse_f32(const float *out, const float *target, const float *mask, int C, int64_t P,
                                  float *gout, double *loss_acc, void *stream) {
    return lrs_masked_mse_cmask_f32(out, target, mask, 1, C, P, gout, loss_acc, stream);
}

extern "C" int lrs_unfolded_to_image_f32(const float *X, const float *L, float c, int64_t H, int64_t W, int64_t B,
                                         float *img, void *stream) {
    if (!X || !img || H <= 0 || W <= 0 || B <= 0) return LRS_E_INVALID;
    hipLaunchKernelGGL(k_unfolded_to_image, dim3(ew_blocks(H * W * B, 8192)), dim3(kEw), 0, (hipStream_t)stream, X,
                       L, c, H, W, B, img);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

extern "C" int lrs_image_to_unfolded_f32(const float *img, int64_t H, int64_t W, int64_t B, float *X, void *stream) {
    if (!X || !img || H <= 0 || W <= 0 || B <= 0) return LRS_E_INVALID;
    hipLaunchKernelGGL(k_image_to_unfolded, dim3(ew_blocks(H * W * B, 8192)), dim3(kEw), 0, (hipStream_t)stream,
                       img, H, W, B, X);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// a frame ReflectionPad2d accepts: the image inside it, every pad smaller than the dimension it mirrors
static bool frame_ok(int64_t H, int64_t W, int64_t top, int64_t left, int64_t Hf, int64_t Wf) {
    return H > 0 && W > 0 && top >= 0 && left >= 0 && top + H <= Hf && left + W <= Wf && Hf <= INT32_MAX / 4 &&
           Wf <= INT32_MAX / 4 && top < H && Hf - H - top < H && left < W && Wf - W - left < W;
}

static dim3 frame_grid(int64_t H, int64_t W, int64_t B) {
    return dim3((unsigned)((W + kFrTile - 1) / kFrTile), (unsigned)((B + kFrTile - 1) / kFrTile), (unsigned)H);
}

extern "C" int lrs_unfolded_to_frame_f32(const float *X, const float *L, float c, int64_t H, int64_t W, int64_t B,
                                         int64_t top, int64_t left, int64_t Hf, int64_t Wf, float *img, void *stream) {
    if (!X || !img || B <= 0 || !frame_ok(H, W, top, left, Hf, Wf)) return LRS_E_INVALID;
    if (H > 65535 || (B + kFrTile - 1) / kFrTile > 65535) return LRS_E_UNSUPPORTED;
    const FrameGeom g{(int)H, (int)W, (int)B, (int)top, (int)left, (int)Hf, (int)Wf};
    hipLaunchKernelGGL(k_unfolded_to_frame, frame_grid(H, W, B), dim3(kFrTile, 8), 0, (hipStream_t)stream, X, L, c, g,
                       img);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

extern "C" int lrs_frame_to_unfolded_f32(const float *img, int64_t H, int64_t W, int64_t B, int64_t top, int64_t left,
                                         int64_t Hf, int64_t Wf, float *X, void *stream) {
    if (!X || !img || B <= 0 || !frame_ok(H, W, top, left, Hf, Wf)) return LRS_E_INVALID;
    if (H > 65535 || (B + kFrTile - 1) / kFrTile > 65535) return LRS_E_UNSUPPORTED;
    const FrameGeom g{(int)H, (int)W, (int)B, (int)top, (int)left, (int)Hf, (int)Wf};
    hipLaunchKernelGGL(k_frame_to_unfolded, frame_grid(H, W, B), dim3(kFrTile, 8), 0, (hipStream_t)stream, img, g, X);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

extern "C" int lrs_es_init(lrs_es_state *st, int size, int patience, void *stream) {
    if (!st || size <= 0 || patience <= 0) return LRS_E_INVALID;
    hipLaunchKernelGGL(k_es_init, dim3(1), dim3(1), 0, (hipStream_t)stream, st, size, patience);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

extern "C" size_t lrs_es_ring_bytes(int size, int64_t N) {
    if (size <= 0 || N <= 0) return 0;
    return (size_t)(es_ab_offset_bytes(size, N) + N * 8 + (2 * kEsMaxBlocks + 2) * 8);
}

extern "C" int lrs_es_update_f32(const float *out, int64_t N, float *ring, lrs_es_state *st, void *stream) {
    if (!out || !ring || !st || N <= 0) return LRS_E_INVALID;
    return es_update(out, N, ring, st, (hipStream_t)stream);
}

// ============================================================================================
// Network engine (the net, its layout and the per-node plan: dipnet_plan.h)
// ============================================================================================
namespace {

// workgroups per conv of the per-step weight preparation
constexpr int kPrepWg = 512;

// raw_first (dipnet_step's overlapped sigma, lrs_dipnet::sn_overlap): the spectral-norm chain and
// the weight preparation were enqueued by the caller (the first conv's planes from the raw weights on
// st, the rest on the side stream, which records ev_sigma); the first conv runs on the raw planes and
// st waits for ev_sigma before its BatchNorm kernel, which divides by the scale.
int dipnet_forward(lrs_dipnet *net, const float *x, hipStream_t st, bool step_begin = false, bool raw_first = false,
                   const PwHead *head = nullptr) {
    int rc;
    if (net->n_sn && !raw_first) {
        rc = sn_launch(net->table(), net->n_sn, net->max_w, net->gram(), net->f(net->sigma_off),
                       net->f(net->scale_off), net->ln_lambda, false, st);
        if (rc) return rc;
    }
    if (net->n_prep && !raw_first) {   // W / scale and the bf16 planes of every conv, one launch
        hipLaunchKernelGGL(k_conv_prep, dim3(kPrepWg, net->n_prep), dim3(256), 0, st, net->prep(), net->f(net->scale_off),
                           step_begin ? net->loss_acc() : nullptr, net->step());
        LRS_CHECK_LAUNCH();
    }
    bool prep_waited = !raw_first;
    for (size_t i = 0; i < net->nodes.size(); ++i) {
        auto &N = net->nodes[i];
        float *out = net->f(N.out_off);
        if (!prep_waited && i > 0) {   // every later node may read the side stream's planes / W / scale
            const hipError_t e = hipStreamWaitEvent(st, net->ev_prep, 0);
            if (e != hipSuccess) return (int)e;
            prep_waited = true;
        }
        if (has_conv(N)) {
            const NodePlan &pl = N.plan;
            // z: the product (the output itself where neither a BatchNorm nor a stage tail reads it)
            float *z = N.z_off >= 0 ? net->f(N.z_off) : out, *part = net->f(net->part_off);
            const float *xin = net->tensor(N.d.in0, x), *w = net->conv_w(N).w, *bias = net->bias_in(net->params, N);
            const __bf16 *wp = N.wpre_off >= 0 ? net->at<__bf16>(N.wpre_off) : nullptr;
            // these BatchNorm kernels finish the product's split-K sum themselves
            int nsplit = 1;
            int *ns = (pl.bn == BnFwd::Reg || pl.bn == BnFwd::Reduce1) ? &nsplit : nullptr;
            rc = LRS_OK;
            switch (pl.fwd) {
            case Fwd::Direct: dir_launch(N.g, pl.dg, xin, w, bias, net->bn_args(N, 0), st); break;
            case Fwd::Upc: rc = upc_fwd(N.g, xin, wp, bias, N.C, z, part, net->part_cap, st, ns); break;
            case Fwd::Sm: {
                const int kk = N.g.k * N.g.k, Cp = r16(N.g.Cin);
                rc = sm_launch(SmPre{wp, (int64_t)N.C * kk * Cp, kk * Cp, N.C},
                               SmFwd{xin, N.g.Cin * N.g.Hs * N.g.Ws * 4, N.g, Cp, nullptr}, z, bias, N.C, (int)N.P, kk * Cp,
                               0, part, net->part_cap, st, ns);
                break;
            }
            case Fwd::Planes:
            case Fwd::Col: {
                const bool act_pw = pl.bn == BnFwd::ActInPw;
                rc = conv_fwd(N.g, xin, w, bias, N.C, N.col_off >= 0 ? net->f(N.col_off) : nullptr, z, part, net->part_cap,
                              st, wp, ns, act_pw ? N.d.act : 0, (act_pw && i + 1 == net->nodes.size()) ? head : nullptr);
                break;
            }
            }
            if (rc) return rc;
            // the DECODE stage's tail: a = act([bilinear x2] z); its BatchNorm, if any, has no activation left
            const float *bn_in = z;
            int bn_act = N.d.act;
            if (pl.tail != Tail::None) {
                float *a = pl.tail_bn ? net->f(N.a_off) : out;
                rc = pl.tail == Tail::Up2Act ? up2_fwd(z, N.C, N.g.Ho, N.g.Wo, N.d.act, a, st)
                                             : dec_act_fwd_launch(z, a, (int64_t)N.C * N.P, N.d.act, st);
                if (rc) return rc;
                bn_in = a;
                bn_act = LRS_ACT_NONE;
            }
            // the raw-weight first conv (its product left >= 2 partials: plan_sn_overlap): its BatchNorm
            // kernel divides by the scale
            const float *sdiv = nullptr;
            if (raw_first && i == 0) {
                const hipError_t e = hipStreamWaitEvent(st, net->ev_sigma, 0);
                if (e != hipSuccess) return (int)e;
                sdiv = net->f(net->scale_off) + N.sn_index;
            }
            const float *pp = nsplit > 1 ? (const float *)part : nullptr;
            if (pl.bn == BnFwd::Reg) {
                launch_bn_fwd_r(pl.nq, pp, nsplit, bias, net->bn_args(N, 1), sdiv, st);
            } else if (pl.bn == BnFwd::Reduce1 && nsplit > 1) {
                launch_reduce_bn1(pp, nsplit, bias, net->bn_args(N, 0), sdiv, st);
            } else if (pl.bn == BnFwd::Reduce1 || pl.bn == BnFwd::Generic) {
                rc = net->node_bn_fwd(N, bn_in, bn_act, st);
            }
        } else if (N.d.kind == LRS_NODE_BN) {
            rc = net->node_bn_fwd(N, net->tensor(N.d.in0, x), N.d.act, st);
        } else {
            const int q = N.cg.H * ((N.cg.W + 3) / 4);
            if (N.cg.Ca + N.cg.Cb > 65535 || !al16(out)) return LRS_E_UNSUPPORTED;
            hipLaunchKernelGGL(k_concat_fwd4, dim3((unsigned)((q + 255) / 256), (unsigned)(N.cg.Ca + N.cg.Cb)), dim3(256),
                               0, st, net->tensor(N.d.in0, x), net->tensor(N.d.in1, x), N.cg, out);
            rc = LRS_OK;
        }
        if (rc) return rc;
    }
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// the early-stopping update of this step's output, run beside the backward (dipnet_step)
// (cr: the interior of a framed output, lrs_dipnet_set_frame; NULL without a frame)
struct EsJob { const float *out; int64_t N; float *ring; lrs_es_state *es; const EsCrop *cr; };

// k_mse_head over the last node (conv without BN): gz and the bias gradient of that node, + loss
int mse_head(lrs_dipnet *net, const float *out, const float *target, const float *mask, int64_t mstride,
             hipStream_t st) {
    const auto &N = net->nodes.back();
    float *gz = net->f(N.gz_off);
    const int64_t P = N.P;
    const int vec = (P % 4 == 0 && al16(out) && al16(target) && mask_al16(mask, mstride) && al16(gz)) ? 1 : 0;
    int64_t S = bn_split(P);   // ~4096 pixels per workgroup
    int64_t chunk = (P + S - 1) / S;
    if (vec) chunk = (chunk + 3) & ~(int64_t)3;
    S = (P + chunk - 1) / chunk;
    // partials: bias [C][S], loss [C][S], channel losses [C]  (bn_part_doubles = 3 C bn_split(P))
    if (chunk > INT32_MAX || P > INT32_MAX || 2 * (int64_t)N.C * S + N.C > bn_part_doubles(N.C, P))
        return LRS_E_UNSUPPORTED;
    if (!net->framed)
        hipLaunchKernelGGL(k_mse_head, dim3((unsigned)S, (unsigned)N.C), dim3(256), 0, st, out, target, mask, mstride, N.C,
                           P, (int)chunk, vec, N.d.act, gz, net->loss_acc(), net->bnpart(), net->headcnt(),
                           net->head_gbias(N));
    else
        hipLaunchKernelGGL(k_mse_head_n, dim3((unsigned)S, (unsigned)N.C), dim3(256), 0, st, out, target, mask, mstride,
                           N.C, P, (int)chunk, vec, N.d.act, gz, net->loss_acc(), net->bnpart(), net->headcnt(),
                           net->head_gbias(N), net->n_mean());
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// Backward from dL/d(output) already in the last node's gradient buffer: every parameter
// gradient into net->grads (the input gets none: the reference's DIP input needs no gradient).
// Weight gradient of conv node i on stream ws: reads dL/dz, the layer input and the scale only.
// scratch: its split-K partials (part2 on the side stream; part on the main one)
// split-K workgroup target of the weight gradients on the side stream: fewer splits would write fewer
// partials and hold fewer CUs beside the data-gradient chain (at most the 512 the workspace is sized for)
constexpr int kWgradSplitWg = 512;

int weight_grad(lrs_dipnet *net, int i, const float *x, hipStream_t ws, float *scratch, int *wsplit_out = nullptr) {
    if (wsplit_out) *wsplit_out = 1;
    const int wt = ws == net->side ? kWgradSplitWg : 512;
    auto &N = net->nodes[i];
    const int t = N.d.in0;
    const float *gz = net->f(N.gz_off), *xin = net->tensor(t, x);
    float *gw = net->grads + N.w_off;
    const lrs_dipnet::ConvW cw = net->conv_w(N);
    const int P = (int)N.P;
    switch (N.plan.wgrad) {
    case Wgrad::Table:   // implicit col^T on k_conv_sm (SmWgrad), dW / scale in its epilogue
        return sm_launch(SmDense{gz, P, N.C},
                         SmWgrad{xin, N.g.Cin * N.g.Hs * N.g.Ws * 4, (int)N.Kc, N.g.k * N.g.k, P, N.g.Hs * N.g.Ws * 4,
                                 net->at<const int>(N.wtab_off)},
                         gw, nullptr, N.C, (int)N.Kc, P, 0, scratch, net->part_cap, ws, nullptr, cw.div, true);
    case Wgrad::Upc: return upc_wgrad(N.g, gz, xin, cw.div, N.C, gw, scratch, net->part_cap, ws, wt);
    case Wgrad::Im2colGemm: {   // the forward gathered inside k_conv_sm: the col for the weight gradient now
        const dim3 grid((unsigned)((P + 255) / 256), (unsigned)std::min<int64_t>(N.Kc, 65535));
        hipLaunchKernelGGL(k_im2col, grid, dim3(256), 0, ws, xin, N.g, net->f(N.col_off));
        break;
    }
    case Wgrad::Gemm: break;
    }
    // explicit: on the node's col buffer; implicit (no col buffer): col^T gathered from the input
    return conv_wgrad(N.g, gz, N.col_off >= 0 ? net->f(N.col_off) : xin, cw.div, N.C, gw, scratch, net->part_cap, ws,
                      N.col_off < 0, wsplit_out, wt);
}

// pw (lrs_dipnet_train_steps): the input conv's weight gradient may leave its split-K partials for
// k_adam to finish (AdamPend; pw->part == nullptr when nothing is pending)
int dipnet_backward(lrs_dipnet *net, const float *x, hipStream_t st, bool head_done = false, AdamPend *pw = nullptr,
                    bool head_reduce = false, const EsJob *esj = nullptr) {
    int rc;
    const int n = (int)net->nodes.size();
    // the ES update reads only the forward's output and its own ring: on the side stream with the first
    // weight gradients (its ring slot and window sums follow the previous step's there), joined before Adam
    auto es_side = [&](hipStream_t hs) -> int {
        if (!esj) return LRS_OK;
        const int r = es_update(esj->out, esj->N, esj->ring, esj->es, hs, esj->cr);
        esj = nullptr;
        return r;
    };
    // the fused loss head's sums (PwHead): the bias gradient of the last conv (read by Adam only) and the
    // loss, on the side stream with the first weight gradient (or here, where none forks)
    auto head_sums = [&](hipStream_t hs) {
        if (!head_reduce) return;
        const auto &Lh = net->nodes[n - 1];
        hipLaunchKernelGGL(k_head_reduce, dim3((unsigned)Lh.C), dim3(256), 0, hs, (const double *)net->hpart(), Lh.C,
                           net->head_nwg, net->head_gbias(Lh), net->closs());
        hipLaunchKernelGGL(k_head_loss, dim3(1), dim3(64), 0, hs, (const double *)net->closs(), Lh.C, net->loss_acc());
        head_reduce = false;
    };
    // gradient buffers: the first contribution to a tensor writes, later ones accumulate
    std::vector<char> written(n + 1, 0);
    written[n] = 1;
    int first_conv = 0;
    while (first_conv < n && !has_conv(net->nodes[first_conv])) ++first_conv;
    // conv node j's weight gradient on the side stream, forked right after its BN backward (its dL/dz is
    // complete by then).  Until round 5 a run of small maps forked every second conv (a fork cost the
    // critical stream ~7 us with system-scope events); with the device-scope events (ensure_side) forking
    // at every conv is faster at both sizes: 196^2 1.192 -> 1.189 ms, 36^2 0.584 -> 0.580 ms (3 interleaved
    // rounds, profiles/r06/ab/fork_sets.txt).
    auto fork_w = [&](int j) -> int {
        hipError_t e = hipEventRecord(net->ev_fork[j], st);
        if (e == hipSuccess) e = hipStreamWaitEvent(net->side, net->ev_fork[j], 0);
        if (e != hipSuccess) return (int)e;
        head_sums(net->side);
        if (const int r = es_side(net->side)) return r;
        return weight_grad(net, j, x, net->side, net->f(net->part2_off));
    };
    // a small-map data gradient may leave dL/dy of the next node as split-K partials, finished by
    // that node's BatchNorm backward (launch_reduce_bn_bwd1; pend = the partials, pend_S their count)
    const float *pend = nullptr;
    int pend_S = 0;
    for (int i = n - 1; i >= 0; --i) {
        auto &N = net->nodes[i];
        float *gout = net->f(N.grad_off);
        if (!written[i + 1]) continue;   // output unused by the loss (cannot happen for a valid net)
        if (has_conv(N)) {
            const NodePlan &pl = N.plan;
            const float *outp = net->f(N.out_off);
            float *gz = net->f(N.gz_off);
            if (pl.tail != Tail::None) {
                // dL/dz on the conv's map: [BatchNorm backward on a ->] the tail's adjoint with the
                // activation's derivative
                const float *ga = gout, *a = outp;
                if (pl.tail_bn) {
                    a = net->f(N.a_off);
                    if ((rc = net->node_bn_bwd(N, a, LRS_ACT_NONE, net->f(N.ga_off), 0, st))) return rc;
                    ga = net->f(N.ga_off);
                }
                rc = pl.tail == Tail::Up2Act ? up2_bwd(ga, a, N.C, N.g.Ho, N.g.Wo, N.d.act, gz, st)
                                             : dec_act_bwd_launch(ga, a, gz, (int64_t)N.C * N.P, N.d.act, st);
                if (rc) return rc;
            } else if (pend) {
                launch_reduce_bn_bwd1(pend, pend_S, net->bn_bwd_args(N), st);
                pend = nullptr;
            } else if (!(head_done && i == n - 1)) {   // else the loss head wrote gz and the bias gradient
                rc = net->node_bn_bwd(N, N.z_off >= 0 ? net->f(N.z_off) : outp, N.d.act, gz, 0, st);
                if (rc) return rc;
            }
            const int t = N.d.in0;
            const lrs_dipnet::ConvW cw = net->conv_w(N);
            float *gx = t > 0 ? net->f(net->nodes[t - 1].grad_off) : nullptr, *part = net->f(net->part_off);
            const __bf16 *wp = N.wpre_off >= 0 ? net->at<const __bf16>(N.wpre_off) : nullptr;
            // weight gradient on the side stream (reads gz, the layer input and the scale only)
            if (!(t == 0 && i == first_conv)) {
                if ((rc = fork_w(i))) return rc;
            } else {
                // the first conv on the input, after which the main stream has no work left of its own (a
                // fork there only adds the event latency to the step's tail); it uses the main stream's
                // scratch, free by then, beside whatever the side stream still runs
                int wsplit = 1;
                const bool defer = pw != nullptr;
                if ((rc = weight_grad(net, i, x, st, part, defer ? &wsplit : nullptr))) return rc;
                if (defer && wsplit > 1) *pw = AdamPend{part, wsplit, N.w_off, (int64_t)N.C * N.Kc, cw.div, net->grads};
            }
            rc = LRS_OK;
            switch (N.plan.dgrad) {
            case Dgrad::None: break;
            case Dgrad::Upc:   // by output parity class over the extended source grid, then the clamp fold
                rc = upc_dgrad(N.g, gz, wp + wprep_elems(N.g, N.C, true).fwd, N.C, gx, net->f(net->dcol_off), part,
                               net->part_cap, st, written[t]);
                break;
            case Dgrad::Adjoint: {   // gx = the adjoint gather of dL/dz on k_conv_sm, one GEMM
                const auto &g = N.g;
                const int kk = g.k * g.k, Cop = r16(N.C);
                const SmPre la{wp + wprep_elems(g, N.C, false).fwd, (int64_t)g.Cin * kk * Cop, kk * Cop, g.Cin};
                // the next node (t - 1 = i - 1, this tensor's only other writer would come before it)
                // finishes the split-K sum inside its BN backward when that fits one workgroup
                const bool fuse_next = t == i && !written[t] && net->nodes[t - 1].plan.bn_bwd_fuse;
                int nsplit = 1;
                rc = sm_launch(la, SmAdj{gz, (int)(N.C * N.P * 4), g, N.C, Cop, net->at<const int4>(N.adj_off), nullptr}, gx,
                               nullptr, g.Cin, g.Hs * g.Ws, kk * Cop, written[t], part, net->part_cap, st,
                               fuse_next ? &nsplit : nullptr);
                if (fuse_next && nsplit > 1) {
                    pend = part;
                    pend_S = nsplit;
                }
                break;
            }
            case Dgrad::Gemm:
                rc = conv_dgrad(N.g, gz, cw.w, N.C, gx, !plain_unit(N.g) ? net->f(net->dcol_off) : nullptr, part,
                                net->part_cap, st, written[t], N.col_off < 0, wp);
                break;
            }
            if (rc) return rc;
            if (t > 0) written[t] = 1;
        } else if (N.d.kind == LRS_NODE_BN) {
            const int t = N.d.in0;
            // (BN straight on the input: parameter grads only, dL/dx into the scratch dz)
            float *gx = t > 0 ? net->f(net->nodes[t - 1].grad_off) : net->f(net->dz_off);
            if ((rc = net->node_bn_bwd(N, net->tensor(t, x), N.d.act, gx, t > 0 ? written[t] : 0, st))) return rc;
            if (t > 0) written[t] = 1;
        } else {
            const int ta = N.d.in0, tb = N.d.in1;
            float *ga = ta > 0 ? net->f(net->nodes[ta - 1].grad_off) : nullptr;
            float *gb = tb > 0 ? net->f(net->nodes[tb - 1].grad_off) : nullptr;
            const int64_t na = ga ? (int64_t)N.cg.Ca * N.cg.Ha * N.cg.Wa : 0;
            const int64_t nb = gb ? (int64_t)N.cg.Cb * N.cg.Hb * N.cg.Wb : 0;
            if (na + nb > 0) {
                const int acc_a = ta > 0 ? written[ta] : 0;
                // both inputs may be the same tensor: the b pass must then accumulate onto the a pass
                const int acc_b = tb > 0 ? (written[tb] || (tb == ta)) : 0;
                // a then b (the same order as one launch over both when ta == tb)
                const CatGeom &cg = N.cg;
                if (ga) {
                    if (!al16(ga)) return LRS_E_UNSUPPORTED;
                    const int q = cg.Ha * ((cg.Wa + 3) / 4);
                    hipLaunchKernelGGL(k_concat_bwd4, dim3((unsigned)((q + 255) / 256), (unsigned)cg.Ca), dim3(256), 0,
                                       st, gout, cg, ga, acc_a, 0);
                }
                if (gb) {
                    if (!al16(gb)) return LRS_E_UNSUPPORTED;
                    const int q = cg.Hb * ((cg.Wb + 3) / 4);
                    hipLaunchKernelGGL(k_concat_bwd4, dim3((unsigned)((q + 255) / 256), (unsigned)cg.Cb), dim3(256), 0,
                                       st, gout, cg, gb, (ta == tb && ga) ? 1 : acc_b, 1);
                }
            }
            if (ta > 0) written[ta] = 1;
            if (tb > 0) written[tb] = 1;
        }
    }
    {   // join the side stream before anyone reads the weight gradients
        hipError_t e = hipEventRecord(net->ev_join, net->side);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, net->ev_join, 0);
        if (e != hipSuccess) return (int)e;
    }
    head_sums(st);   // (only if no fork took them)
    if ((rc = es_side(st))) return rc;
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// mstride: the mask's row stride (mask_stride: 0 for a [P] mask or none, P for a [C][P] one)
int dipnet_step(lrs_dipnet *net, const float *x, const float *target, const float *mask, int64_t mstride, float lr,
                float b1, float b2, float eps, lrs_es_state *es, float *ring, hipStream_t st) {
    // the weight-preparation launch at the head of the forward also zeroes the loss accumulator
    // and advances Adam's step counter (read only by this step's k_adam); without one, a tiny launch
    const bool folded = net->n_prep > 0;
    // (sn_overlap: decided at bind from the first conv's plan, plan_sn_overlap)
    const bool overlap = net->sn_overlap && net->side && net->ev_head && net->ev_sigma && net->ev_prep;
    if (overlap) {
        // the spectral-norm Grams here (alone they take 19 us at 196^2; on the side stream beside the
        // first conv, 50), then the rest of the chain (Gram reduce, Lanczos) and the preparation of every
        // conv but the first on the side stream beside the first conv, whose planes come from the raw
        // weights here
        // (the Gram reduce too: on the side stream beside the first conv it took 23 us instead of 6)
        hipLaunchKernelGGL(k_sn_gram_head, dim3(kSnSplit, net->n_sn + kHeadPlaneRows), dim3(256), 0, st, net->table(), net->gram(),
                           net->n_sn, (const ConvPrep *)net->prep_head(), net->loss_acc(), net->step());
        hipLaunchKernelGGL(k_sn_gram_reduce, dim3(kSnPairs, net->n_sn), dim3(256), 0, st, net->table(), net->gram());
        hipError_t e = hipEventRecord(net->ev_head, st);
        if (e == hipSuccess) e = hipStreamWaitEvent(net->side, net->ev_head, 0);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(k_sn_sigma, dim3(net->n_sn), dim3(256), 0, net->side, net->table(), net->gram(),
                           net->f(net->sigma_off), net->f(net->scale_off), net->ln_lambda, (long long *)nullptr);
        // the first BatchNorm waits for the scale only, the second conv for the planes as well: 196^2 step
        // 1.185 -> 1.179 ms against one event after both (3 interleaved rounds,
        // profiles/r06/ab/split_event_and_es.txt)
        if ((e = hipEventRecord(net->ev_sigma, net->side)) != hipSuccess) return (int)e;
        if (net->n_prep)
            hipLaunchKernelGGL(k_conv_prep, dim3(kPrepWg, net->n_prep), dim3(256), 0, net->side, net->prep_side(),
                               net->f(net->scale_off), (double *)nullptr, net->step());
        if ((e = hipEventRecord(net->ev_prep, net->side)) != hipSuccess) return (int)e;
        LRS_CHECK_LAUNCH();
    }
    const int n = (int)net->nodes.size();
    const auto &Lst = net->nodes[n - 1];
    // the loss head in the last conv's epilogue (k_pw): gz, and per-workgroup sums for the bias gradient
    // and the loss, reduced in the backward on the side stream (k_mse_head's arithmetic per element)
    const PwHead hd{target, mask, mstride, net->f(Lst.gz_off), net->hpart(),
                    net->framed ? (float)(2.0 / (double)net->n_mean())
                                : (float)(2.0 / ((double)Lst.C * (double)Lst.P)),
                    &net->head_nwg};
    // (k_pw's epilogue takes its float4 form when P % 4 == 0 and reads the mask rows as float4 there;
    // a [C][P] mask with P % 4 != 0 has unaligned rows and takes k_mse_head's scalar path instead)
    const bool fused_head = net->head_pw && mask_al16(mask, mstride) && al16(target);
    int rc = dipnet_forward(net, x, st, folded, overlap, fused_head ? &hd : nullptr);
    if (rc) return rc;
    const float *out = net->f(Lst.out_off);
    if (!folded) hipLaunchKernelGGL(k_step_begin, dim3(1), dim3(64), 0, st, net->loss_acc(), net->step());
    if (fused_head) {
        rc = LRS_OK;
    } else if (net->head_fusable) {
        rc = mse_head(net, out, target, mask, mstride, st);
    } else {
        rc = masked_mse(out, target, mask, mstride ? Lst.C : 1, Lst.C, Lst.P, net->n_mean(), net->f(Lst.grad_off),
                        net->loss_acc(), st);
    }
    if (rc) return rc;
    // the input conv's weight-gradient split-K sum is finished inside Adam (one launch less on the
    // step's tail)
    AdamPend pw{};
    // (the early-stopping ring holds the interior of a framed output only: what the frame holds is
    // constrained by nothing and must not drive the stop)
    const EsCrop crop{net->fr_top, net->fr_left, net->fr_H, net->fr_W, Lst.H, Lst.W};
    const EsJob esj{out, net->n_mean(), ring, es, net->framed ? &crop : nullptr};
    rc = dipnet_backward(net, x, st, net->head_fusable, &pw, fused_head, es ? &esj : nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(k_adam, dim3(ew_blocks((net->n_params + 3) / 4, 8192)), dim3(kEw), 0, st, net->params,
                       (const float *)net->grads, net->am, net->av, net->n_params, (const int *)net->step(), lr, b1, b2,
                       eps, pw);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// The side streams and the fork/join events are created on the first training call that needs
// them (outside any capture), so that creating a net and querying its layout needs no device.
// The side stream takes the priority of the calling stream, so a caller that trains the net on a
// high-priority stream (LrsPnPConfig.lowrank_priority) gets its weight gradients placed with the
// same priority.  One side stream is kept per priority seen (at most two in practice), so a call
// on a stream of another priority only selects a different one: no host synchronisation and no
// graph drop (a captured graph holds its own nodes, not the stream).
int ensure_side(lrs_dipnet *net, hipStream_t st) {
    int prio = 0;
    hipError_t e = hipStreamGetPriority(st, &prio);
    if (e != hipSuccess) return (int)e;
    for (auto &ps : net->sides)
        if (ps.first == prio) {
            net->side = ps.second;
            return LRS_OK;
        }
    hipStream_t s = nullptr;
    e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio);
    if (e != hipSuccess) return (int)e;
    net->sides.emplace_back(prio, s);
    net->side = s;
    // The fork / join events only order kernels of this device against each other (nothing on the host
    // waits on them), so they are recorded with device-scope fences -- what a kernel boundary inside one
    // stream has -- instead of the default system-scope release, whose cache write-back the critical
    // stream paid at every fork (tools/micro/fork_cost: DESIGN.md §5).
    constexpr unsigned evf = hipEventDisableTiming | hipEventDisableSystemFence;
    for (hipEvent_t *ev : {&net->ev_join, &net->ev_head, &net->ev_sigma, &net->ev_prep})
        if (e == hipSuccess && !*ev) e = hipEventCreateWithFlags(ev, evf);
    for (size_t i = 0; i < net->ev_fork.size() && e == hipSuccess; ++i)
        if (!net->ev_fork[i]) e = hipEventCreateWithFlags(&net->ev_fork[i], evf);
    return (int)e;
}

void drop_graph(lrs_dipnet *net) {
    if (net->gexec) (void)hipGraphExecDestroy(net->gexec);
    if (net->graph) (void)hipGraphDestroy(net->graph);
    net->gexec = nullptr; net->graph = nullptr; net->have_key = false;
}

}  // namespace

extern "C" int lrs_dipnet_create(const lrs_dip_node *nodes, int n_nodes, int C, int H, int W,
                                 const lrs_dip_opts *opts, lrs_dipnet **out) {
    if (!nodes || n_nodes <= 0 || C <= 0 || H <= 0 || W <= 0 || !out) return LRS_E_INVALID;
    const lrs_dip_opts o = dip_opts(opts);
    if (!dip_opts_ok(o)) return LRS_E_INVALID;
    lrs_dipnet *net = new (std::nothrow) lrs_dipnet();
    if (!net) return LRS_E_INVALID;
    net->C0 = C; net->H = H; net->W = W;
    net->opts = o;
    net->implicit = o.precision == LRS_DIP_SPLIT_BF16;
    if (const int rc = dipnet_layout(net, nodes, n_nodes)) {
        delete net;
        return rc;
    }
    net->fr_H = net->nodes.back().H;   // no frame: the whole output
    net->fr_W = net->nodes.back().W;
    *out = net;
    return LRS_OK;
}

extern "C" void lrs_dipnet_destroy(lrs_dipnet *net) {
    if (!net) return;
    drop_graph(net);
    for (auto &ps : net->sides) (void)hipStreamSynchronize(ps.second);
    for (hipEvent_t ev : net->ev_fork)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : {net->ev_join, net->ev_head, net->ev_sigma, net->ev_prep})
        if (ev) (void)hipEventDestroy(ev);
    for (auto &ps : net->sides) (void)hipStreamDestroy(ps.second);
    delete net;
}

extern "C" int64_t lrs_dipnet_num_params(const lrs_dipnet *net) { return net ? net->n_params : -1; }
extern "C" int64_t lrs_dipnet_num_bnstats(const lrs_dipnet *net) { return net ? net->n_bnstats : -1; }
extern "C" size_t lrs_dipnet_workspace(const lrs_dipnet *net) { return net ? net->ws_bytes : 0; }

extern "C" int lrs_dipnet_param_offsets(const lrs_dipnet *net, int node, int64_t *w, int64_t *b, int64_t *gamma,
                                        int64_t *beta) {
    if (!net || node < 0 || node >= (int)net->nodes.size()) return LRS_E_INVALID;
    const auto &N = net->nodes[node];
    if (w) *w = N.w_off; if (b) *b = N.b_off;
    if (gamma) *gamma = N.gm_off; if (beta) *beta = N.bt_off;
    return LRS_OK;
}

extern "C" int lrs_dipnet_node_shape(const lrs_dipnet *net, int node, int *C, int *H, int *W) {
    if (!net || node < -1 || node >= (int)net->nodes.size()) return LRS_E_INVALID;
    const int t = node + 1;
    if (C) *C = net->tC(t); if (H) *H = net->tH(t); if (W) *W = net->tW(t);
    return LRS_OK;
}

extern "C" int lrs_dipnet_out_shape(const lrs_dipnet *net, int *C, int *H, int *W) {
    if (!net) return LRS_E_INVALID;
    return lrs_dipnet_node_shape(net, (int)net->nodes.size() - 1, C, H, W);
}

extern "C" int lrs_dipnet_bind(lrs_dipnet *net, float *params, float *grads, float *adam_m, float *adam_v,
                               float *bnstats, void *ws, size_t ws_bytes) {
    if (!net || !params || !grads || !adam_m || !adam_v || (!bnstats && net->n_bnstats)) return LRS_E_INVALID;
    if (!ws || ws_bytes < net->ws_bytes) return LRS_E_WORKSPACE;
    drop_graph(net);
    net->params = params; net->grads = grads; net->am = adam_m; net->av = adam_v;
    net->bnstats = bnstats; net->ws = (char *)ws;
    plan_bind(net);
    std::vector<SnConv> tab;
    for (const auto &N : net->nodes)
        if (N.sn_index >= 0) tab.push_back(SnConv{params + N.w_off, net->f(N.wn_off), N.C, (int)N.Kc});
    std::vector<ConvPrep> prep;
    for (size_t i = 0; i < net->nodes.size(); ++i) {
        const auto &N = net->nodes[i];
        if (!has_conv(N) || (N.sn_index < 0 && N.wpre_off < 0)) continue;
        __bf16 *wf = N.wpre_off >= 0 ? net->at<__bf16>(N.wpre_off) : nullptr;
        __bf16 *wd = (wf && N.d.in0 > 0) ? wf + wprep_elems(N.g, N.C, N.upc).fwd : nullptr;
        prep.push_back(ConvPrep{params + N.w_off, N.sn_index >= 0 ? net->f(N.wn_off) : nullptr, wf, wd, N.C, N.g.Cin,
                                N.g.k * N.g.k, r16(N.g.Cin), r16(N.C), N.sn_index, N.g.k,
                                (wd && !N.sm && !N.upc) ? N.g.ke : 0, N.upc ? 1 : 0});
    }
    hipError_t e = hipSuccess;
    for (const auto &N : net->nodes) {
        if (e == hipSuccess && N.sm_dgrad)
            e = hipMemcpy(net->f(N.adj_off), N.adj.data(), sizeof(int) * N.adj.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess && N.wtab_off >= 0)
            e = hipMemcpy(net->f(N.wtab_off), N.wtab.data(), sizeof(int) * N.wtab.size(), hipMemcpyHostToDevice);
    }
    if (!tab.empty()) e = hipMemcpy(net->table(), tab.data(), sizeof(SnConv) * tab.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && !prep.empty())
        e = hipMemcpy(net->prep(), prep.data(), sizeof(ConvPrep) * prep.size(), hipMemcpyHostToDevice);
    if (net->sn_overlap && !prep.empty()) {
        // head: the first conv's forward planes from the raw weights (si = -1: no division, no W / s);
        // side: every entry, the first conv's without its planes (the main stream reads them meanwhile)
        ConvPrep head = prep[0], side0 = prep[0];
        head.Wn = nullptr;
        head.wd = nullptr;
        head.si = -1;
        side0.wf = nullptr;
        side0.wd = nullptr;
        std::vector<ConvPrep> side(prep);
        side[0] = side0;
        static_assert(sizeof(ConvPrep) <= 256, "one ConvPrep in the head slot");
        if (e == hipSuccess) e = hipMemcpy(net->prep_head(), &head, sizeof(ConvPrep), hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpy(net->prep_side(), side.data(), sizeof(ConvPrep) * side.size(), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipMemset(net->ws + net->misc_off, 0, 256);
    if (e == hipSuccess) e = hipMemset(net->headcnt(), 0, sizeof(int) * (net->nodes.back().C + 1));
    return e == hipSuccess ? LRS_OK : (int)e;
}

extern "C" int lrs_dipnet_init_params(lrs_dipnet *net, uint64_t seed, void *stream) {
    if (!net || !net->params) return LRS_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    for (size_t i = 0; i < net->nodes.size(); ++i) {
        const auto &N = net->nodes[i];
        const uint64_t k1 = mix64(seed * 0x100000001b3ULL + 2 * i + 1), k2 = mix64(seed * 0x100000001b3ULL + 2 * i + 2);
        if (has_conv(N)) {
            const float fan_in = (float)N.Kc;
            // kaiming_uniform_(a=0, fan_in) (lipschitz_constraint_layer.py:74) or the nn.Conv2d
            // default kaiming_uniform_(a=sqrt(5)) = U(-1/sqrt(fan_in), +)
            const float wb = N.d.winit == LRS_WINIT_KAIMING ? sqrtf(6.0f / fan_in) : 1.0f / sqrtf(fan_in);
            const float bb = 1.0f / sqrtf(fan_in);
            hipLaunchKernelGGL(k_init_uniform, dim3(ew_blocks(N.C * N.Kc)), dim3(kEw), 0, st, net->params + N.w_off,
                               (int64_t)(N.C * N.Kc), wb, k1);
            if (float *b = net->bias_in(net->params, N))   // (a DECODE stage has no bias)
                hipLaunchKernelGGL(k_init_uniform, dim3(1), dim3(kEw), 0, st, b, (int64_t)N.C, bb, k2);
        }
        if (N.d.bn) {
            hipLaunchKernelGGL(k_fill, dim3(1), dim3(kEw), 0, st, net->params + N.gm_off, (int64_t)N.C, 1.0f);
            hipLaunchKernelGGL(k_fill, dim3(1), dim3(kEw), 0, st, net->params + N.bt_off, (int64_t)N.C, 0.0f);
            hipLaunchKernelGGL(k_fill, dim3(1), dim3(kEw), 0, st, net->bnstats + N.rs_off, (int64_t)N.C, 0.0f);
            hipLaunchKernelGGL(k_fill, dim3(1), dim3(kEw), 0, st, net->bnstats + N.rs_off + N.C, (int64_t)N.C, 1.0f);
        }
    }
    const hipError_t e = hipMemsetAsync(net->grads, 0, sizeof(float) * net->n_params, st);
    if (e != hipSuccess) return (int)e;
    LRS_CHECK_LAUNCH();
    return lrs_dipnet_reset_optimizer(net, stream);   // the Adam moments and the step count
}

extern "C" int lrs_dipnet_reset_optimizer(lrs_dipnet *net, void *stream) {
    if (!net || !net->ws) return LRS_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(net->am, 0, sizeof(float) * net->n_params, st);
    if (e == hipSuccess) e = hipMemsetAsync(net->av, 0, sizeof(float) * net->n_params, st);
    if (e == hipSuccess) e = hipMemsetAsync(net->ws + net->misc_off, 0, 256, st);
    return e == hipSuccess ? LRS_OK : (int)e;
}

extern "C" int lrs_dipnet_forward(lrs_dipnet *net, const float *x, void *stream) {
    if (!net || !net->ws || !x) return LRS_E_INVALID;
    return dipnet_forward(net, x, (hipStream_t)stream);
}

extern "C" int lrs_dipnet_backward(lrs_dipnet *net, const float *x, const float *gout, void *stream) {
    if (!net || !net->ws || !x || !gout) return LRS_E_INVALID;
    if (const int rs = ensure_side(net, (hipStream_t)stream)) return rs;
    hipStream_t st = (hipStream_t)stream;
    const auto &Lst = net->nodes.back();
    const hipError_t e = hipMemcpyAsync(net->f(Lst.grad_off), gout, sizeof(float) * Lst.C * Lst.P,
                                        hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return (int)e;
    return dipnet_backward(net, x, st);
}

extern "C" int lrs_dipnet_set_ln_lambda(lrs_dipnet *net, float ln_lambda) {
    if (!net || !(ln_lambda > 0.0f)) return LRS_E_INVALID;
    drop_graph(net);
    net->ln_lambda = ln_lambda;
    return LRS_OK;
}

extern "C" int lrs_dipnet_set_frame(lrs_dipnet *net, int top, int left, int H, int W) {
    if (!net) return LRS_E_INVALID;
    const auto &Lst = net->nodes.back();
    if (!frame_ok(H, W, top, left, Lst.H, Lst.W)) return LRS_E_INVALID;
    net->fr_top = top; net->fr_left = left; net->fr_H = H; net->fr_W = W;
    net->framed = H != Lst.H || W != Lst.W;   // the whole output: the unframed step, kernel for kernel
    return LRS_OK;
}

extern "C" int lrs_dipnet_get_frame(const lrs_dipnet *net, int *top, int *left, int *H, int *W) {
    if (!net) return LRS_E_INVALID;
    if (top) *top = net->fr_top; if (left) *left = net->fr_left;
    if (H) *H = net->fr_H; if (W) *W = net->fr_W;
    return LRS_OK;
}

extern "C" const float *lrs_dipnet_output(const lrs_dipnet *net) {
    return (net && net->ws) ? net->f(net->nodes.back().out_off) : nullptr;
}

extern "C" const float *lrs_dipnet_grads(const lrs_dipnet *net) { return net ? net->grads : nullptr; }

// Diagnostics: a node's activation buffers in the bound workspace (node's output, its pre-BN z,
// dL/dz, dL/d(output)); NULL where the node has none.  Valid until the next call on the net.
extern "C" const float *lrs_dipnet_node_buffer(const lrs_dipnet *net, int node, int which) {
    if (!net || !net->ws || node < 0 || node >= (int)net->nodes.size()) return nullptr;
    const auto &N = net->nodes[node];
    int64_t off = -1;
    if (which == LRS_BUF_OUT) off = N.out_off;
    else if (which == LRS_BUF_Z) off = N.z_off;
    else if (which == LRS_BUF_GZ) off = N.gz_off;
    else if (which == LRS_BUF_GRAD) off = N.grad_off;
    const bool tail = N.plan.tail != Tail::None;
    if (tail && which == LRS_BUF_Z) off = N.a_off;     // what its BatchNorm reads, at the node's shape
    if (tail && which == LRS_BUF_GZ) off = N.ga_off;   // (z and dL/dz live on the conv's smaller map)
    return off >= 0 ? net->f(off) : nullptr;
}

extern "C" int lrs_dipnet_train_steps_cmask(lrs_dipnet *net, const float *x, const float *target, const float *mask,
                                            int mask_channels, float lr, float beta1, float beta2, float eps,
                                            lrs_es_state *es, float *ring, int nsteps, int use_graph, void *stream) {
    if (!net || !net->ws || !x || !target || nsteps < 0 || (es && !ring)) return LRS_E_INVALID;
    const int64_t mstride = mask_stride(mask, mask_channels, net->nodes.back().C, net->nodes.back().P);
    if (mstride < 0) return LRS_E_INVALID;   // before anything is launched
    hipStream_t st = (hipStream_t)stream;
    if (const int rs = ensure_side(net, (hipStream_t)stream)) return rs;
    if (!use_graph) {
        for (int s = 0; s < nsteps; ++s) {
            const int rc = dipnet_step(net, x, target, mask, mstride, lr, beta1, beta2, eps, es, ring, st);
            if (rc) return rc;
        }
        return LRS_OK;
    }
    if (!st) return LRS_E_INVALID;   // capture needs a non-default stream
    const lrs_dipnet::Key k{x, target, mask, es, ring, mstride, lr, beta1, beta2, eps,
                            net->fr_top, net->fr_left, net->fr_H, net->fr_W};
    static_assert(sizeof(lrs_dipnet::Key) == 5 * sizeof(void *) + sizeof(int64_t) + 4 * sizeof(float) + 4 * sizeof(int32_t),
                  "Key has padding");
    if (!net->have_key || memcmp(&k, &net->key, sizeof(k)) != 0) {
        drop_graph(net);
        hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
        if (e != hipSuccess) return (int)e;
        const int rc = dipnet_step(net, x, target, mask, mstride, lr, beta1, beta2, eps, es, ring, st);
        hipGraph_t g = nullptr;
        e = hipStreamEndCapture(st, &g);
        if (rc) {
            if (g) (void)hipGraphDestroy(g);
            return rc;
        }
        if (e != hipSuccess) return (int)e;
        e = hipGraphInstantiate(&net->gexec, g, nullptr, nullptr, 0);
        if (e != hipSuccess) {
            (void)hipGraphDestroy(g);
            return (int)e;
        }
        net->graph = g;
        net->key = k;
        net->have_key = true;
    }
    for (int s = 0; s < nsteps; ++s) {
        const hipError_t e = hipGraphLaunch(net->gexec, st);
        if (e != hipSuccess) return (int)e;
    }
    return LRS_OK;
}

extern "C" int lrs_dipnet_train_steps(lrs_dipnet *net, const float *x, const float *target, const float *mask,
                                      float lr, float beta1, float beta2, float eps, lrs_es_state *es, float *ring,
                                      int nsteps, int use_graph, void *stream) {
    return lrs_dipnet_train_steps_cmask(net, x, target, mask, 1, lr, beta1, beta2, eps, es, ring, nsteps, use_graph, stream);
}

extern "C" int lrs_dipnet_last_loss(lrs_dipnet *net, double *loss, void *stream) {
    if (!net || !net->ws || !loss) return LRS_E_INVALID;
    double acc = 0.0;
    hipError_t e = hipMemcpyAsync(&acc, net->loss_acc(), sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    *loss = acc / (double)net->n_mean();
    return LRS_OK;
}

extern "C" int lrs_dipnet_get_opts(const lrs_dipnet *net, lrs_dip_opts *opts) {
    if (!net || !opts) return LRS_E_INVALID;
    *opts = net->opts;
    return LRS_OK;
}

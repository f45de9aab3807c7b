// DIP low-rank prox: C-ABI of the layer primitives and the sequential-network training engine.
//
// Reference: main_LRS_PnP_DIP_1-LiP.py:208-264 (get_DIP_out: fresh my_Lipschitz_Unet, Adam,
// masked MSE, early stopping) and models/my_Lipschitz_Unet.py:21-148.  The engine launches one
// training step as ~8 kernels per conv unit from C++ (no per-layer Python), and can capture the
// step in a hipGraph and replay it: the Adam step count and the early-stopping state live in
// device memory, so a replayed step is exactly the eager step.
// dip_launch.h: geometry and the kernel launchers; dipnet_plan.h: the net, its layout and its plans;
// dipnet_engine.h: the forward, the backward and the step; dip_tv.h: the stand-alone TV term of the output
// (lrs_sstv_f32).  This file holds the C entry points.
// Every node with a conv product (CONV, and the Deep Decoder's DECODE) runs one path: product -> the
// stage tail the plan names (DECODE: [bilinear x2 +] activation) -> BatchNorm; a node's generic
// BatchNorm call is lrs_dipnet::node_bn_fwd / node_bn_bwd, a bias that may be absent bias_in.
#include "dipnet_engine.h"
#include "dip_tv.h"

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

extern "C" int lrs_masked_mse_cmask_f32(const float *out, const float *target, const float *mask, int mask_channels,
                                        int C, int64_t P, float *gout, double *loss_acc, void *stream) {
    return masked_mse(out, target, mask, mask_channels, C, P, (int64_t)C * P, gout, loss_acc, stream);
}

extern "C" int lrs_masked_mse_framed_f32(const float *out, const float *target, const float *mask, int mask_channels,
                                         int C, int64_t P, int64_t n_mean, float *gout, double *loss_acc,
                                         void *stream) {
    return masked_mse(out, target, mask, mask_channels, C, P, n_mean, gout, loss_acc, stream);
}

extern "C" int lrs_sstv_f32(const float *out, int C, int Hf, int Wf, int top, int left, int H, int W, float w_sp,
                            float w_bd, float w_ss, float eps, int64_t n_mean, float *gout, double *loss_acc,
                            void *stream) {
    return sstv(out, C, Hf, Wf, top, left, H, W, w_sp, w_bd, w_ss, eps, n_mean, gout, loss_acc, (hipStream_t)stream);
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
// Network engine (dipnet_engine.h; the net, its layout and its plans: dipnet_plan.h)
// ============================================================================================
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
    if (net->step_plan.sn_overlap && !prep.empty()) {
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
    return dipnet_forward(net, x, (hipStream_t)stream, FwdStep{});
}

extern "C" int lrs_dipnet_backward(lrs_dipnet *net, const float *x, const float *gout, void *stream) {
    if (!net || !net->ws || !x || !gout) return LRS_E_INVALID;
    if (const int rs = ensure_side(net, (hipStream_t)stream)) return rs;
    hipStream_t st = (hipStream_t)stream;
    const auto &Lst = net->nodes.back();
    const hipError_t e = hipMemcpyAsync(net->f(Lst.grad_off), gout, sizeof(float) * Lst.C * Lst.P,
                                        hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return (int)e;
    return dipnet_backward(net, x, st, BwdStep{});
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
    if (!net->have_key || memcmp(&k, &net->key, sizeof(k)) != 0)
        if (const int rc = capture_step(net, k, x, target, mask, es, ring, st)) return rc;
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

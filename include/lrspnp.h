/*
 * liblrspnp_hip.so — C ABI of the MI355X-native LRS-PnP inner loop (gfx950 / CDNA4).
 *
 * Plain C: pointers, sizes, a `void *stream` (a hipStream_t, NULL = default stream).  Every
 * device pointer is caller-owned; the library never allocates (workspaces are sized by the
 * `*_workspace` queries and passed in).  Calls are stream-ordered and reentrant, never
 * synchronise the host, and return 0 (LRS_OK), a negative LRS_E_* code, or a positive
 * hipError_t.  Arrays are float32 row-major unless noted.  Modes are per call (lrs_ista_opts,
 * lrs_dip_opts) or per handle; no exported function changes process-wide state.
 *
 * Reference interfaces replaced (shuoli0708/LRS-PnP-DIP; file:line):
 *   lrs_nlm_col_f32       skimage.restoration.denoise_nl_means(g, h, fast_mode=True,
 *                         patch_size=3, patch_distance=3) as called at
 *                         main_LRS_PnP_DIP_1-LiP.py:196, main_LRS_PnP.py:146
 *   lrs_block_count/_grid get_image_block corner logic            main_LRS_PnP.py:73-99
 *   lrs_im2col_f32        get_image_block gather of X + lambda_1/mu_1, plus the missing-pixel
 *                         masks of blocks_copy                     main_LRS_PnP.py:101-105,244,259,278
 *   lrs_ista_alpha_f32    alpha / T / h inside ista()              main_LRS_PnP.py:134-146,
 *                                                                  main_LRS_PnP_DIP_1-LiP.py:187-196
 *   lrs_ista_f32          the per-block loop: delete_element + ista + Phi_z = D @ Coefs,
 *                         for all blocks at once               main_LRS_PnP.py:270-303,131-155
 *   lrs_svt_f32           SVT(X + lambda_2/mu_2, 1/mu_2)          main_LRS_PnP.py:112-124,315
 *   lrs_admm_update_f32   col2im, closed-form X update, dual updates, state_convergence norms
 *                                                                  main_LRS_PnP.py:324-366,23-25
 */
#ifndef LRSPNP_H
#define LRSPNP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LRS_OK 0
#define LRS_E_INVALID (-1)     /* bad argument (shape, null pointer, unsupported parameter) */
#define LRS_E_UNSUPPORTED (-2) /* parameter combination not compiled in (e.g. K) */
#define LRS_E_WORKSPACE (-3)   /* workspace too small */
#define LRS_E_NODEVICE (-4)    /* no gfx950 device */

/* ISTA step-size rule (alpha) and prox */
#define LRS_ALPHA_SPEC2 0 /* alpha = ||H||_2^2, NLM h = 0.1*T   main_LRS_PnP.py:134,146      */
#define LRS_ALPHA_FRO4 1  /* alpha = 4||H||_F^2, NLM h = T      …1-LiP.py:187,196           */
#define LRS_ALPHA_SOFT 2  /* alpha = ||H||_2^2, soft threshold T (ista.m:15-23)              */
#define LRS_PROX_NLM 0
#define LRS_PROX_SOFT 1
#define LRS_PROX_NLM_MATLAB 2 /* NLmeansfilter(g,3,3,0.1T) of pnp_ista.m:30, fp64        */

const char *lrs_version(void);
/* 0 when the current device is gfx950, LRS_E_NODEVICE otherwise. */
int lrs_check_device(void);

/* ---- NLM prox ------------------------------------------------------------------------------
 * out[v*ldo + i] = NLM(g[v*ldg + 0..K-1])[i] for v < nvec.  h_per_vec (device, nvec doubles)
 * overrides h when non-NULL.  Only patch_size = 3, patch_distance = 3 (the reference's call). */
int lrs_nlm_col_f32(const float *g, int64_t ldg, float *out, int64_t ldo, int64_t K, int64_t nvec,
                    double h, const double *h_per_vec, int patch_size, int patch_distance,
                    void *stream);

/* ---- Block grid (host-side) ----------------------------------------------------------------
 * Block corners of get_image_block on a P x B unfolded matrix, in the reference's order
 * (column-major over corners).  rows/cols are host arrays of length lrs_block_count(). */
int64_t lrs_block_count(int64_t P, int64_t B, int64_t bb, int64_t sliding);
int lrs_block_grid(int64_t P, int64_t B, int64_t bb, int64_t sliding, int32_t *rows, int32_t *cols,
                   int64_t nb);
/* For every index x in [0, extent): the contiguous range [lo[x], hi[x]] of positions in the
 * sorted `starts` whose bb-window covers x (hi < lo when none).  Host arrays. */
int lrs_cover_ranges(int64_t extent, int64_t bb, const int32_t *starts, int64_t nstarts,
                     int32_t *lo, int32_t *hi);

/* ---- im2col --------------------------------------------------------------------------------
 * Yb[j*n_pad + a + bb*c] = X[rows[j]+a][cols[j]+c] + L[..]/mu   (L may be NULL: X alone);
 * entries n..n_pad-1 are 0.  obs (nullable, u8 [nb][n_pad]) = 1 where that value != 0.
 * rows/cols are DEVICE int32 arrays. */
int lrs_im2col_f32(const float *X, const float *L, float mu, int64_t P, int64_t B, int64_t bb,
                   const int32_t *rows, const int32_t *cols, int64_t nb, int64_t n_pad, float *Yb,
                   uint8_t *obs, void *stream);

/* ---- ISTA step size / threshold per observation pattern ------------------------------------
 * obs_pat: u8 [npat][n_pad] (1 = observed row).  D: n x K.  Writes alpha_pat[npat] (float32,
 * as numpy returns it) and thr_pat[npat] (the NLM h, or the soft threshold T).
 * SPEC2/SOFT run a fp64 Lanczos on the masked Gram in `ws`. */
size_t lrs_ista_alpha_workspace(int64_t n, int64_t K, int64_t npat);
int lrs_ista_alpha_f32(const float *D, int64_t n, int64_t K, const uint8_t *obs_pat, int64_t npat,
                       int64_t n_pad, int alpha_mode, float lambda_ista, float *alpha_pat,
                       double *thr_pat, void *ws, size_t ws_bytes, void *stream);

/* ---- Masked ISTA with PnP prox over all blocks (the hot kernel) ----------------------------
 * Yb, obs: [nb][n_pad]; D: n x K; alpha[nb], thr[nb].  x0 = 0; Nit iterations of
 *   g = x + D^T(obs .* (y - D x)) / alpha ;  x = prox(g)
 * then phi[j*n_pad + r] = (D x_j)[r] for r < n (all rows, the inpainting step).
 * coefs (nullable) receives x [nb][K].  Any n (n_pad % 16 == 0), any K <= 16384 (K > 512 on the
 * generic dense-GEMM path, see lrs_ista_opts), every prox.
 * n_pad <= 64 with K = 256 runs the dictionary-resident kernels (ws unused); everything else runs
 * the row-split kernel, whose fragment-ordered dictionary images live in `ws`
 * (lrs_ista_workspace bytes; LRS_E_WORKSPACE when too small).
 * Replaces the per-block loop of main_LRS_PnP.py:270-303 / main_LRS_PnP_DIP_1-LiP.py:367-392
 * around ista() (main_LRS_PnP.py:131-149, …1-LiP.py:185-198) and delete_element (:201-204). */
/* Per-call options (NULL = defaults); the library keeps no process-wide mode.
 *   precision: arithmetic of the two products of the resident (n_pad <= 64) kernel:
 *     LRS_ISTA_SPLIT_BF16 (default): bf16 matrix cores on operands split exactly into three bf16
 *     terms (six partial products, fp32 accumulation: fp32-GEMM accuracy, not bitwise the f32
 *     MFMA); LRS_ISTA_F32: v_mfma_f32_16x16x4_f32 (exact f32 products).  The NLM prox is identical.
 *   max_workgroups: 0 (default) = one workgroup per 16-block tile; > 0 bounds the row-split
 *     kernel's grid (each workgroup then loops over tiles), so a concurrent launch on another
 *     stream (the DIP training of the …_DIP mains) keeps the rest of the CUs.  Results do not
 *     depend on it.
 *   accel: LRS_ISTA_ACCEL_NONE (0, default): the reference's ISTA above.  LRS_ISTA_ACCEL_FISTA: the
 *     same gradient step and prox with Nesterov / FISTA momentum.  Start with x_0 (zero, or coefs
 *     under warm_start), z_1 = x_0, t_1 = 1.  For k = 1..Nit:
 *       x_k     = prox(z_k + D^T(obs .* (y - D z_k)) / alpha)
 *       t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2
 *       beta_k  = (t_k - 1) / t_{k+1}
 *       z_{k+1} = x_k + beta_k (x_k - x_{k-1})
 *     t and beta are computed in fp64 and beta is rounded once to float32; z is formed in float32.
 *     The result is x_Nit, never z: the last iteration writes x itself back, and coefs and
 *     phi = D x_Nit are formed from x_Nit.  alpha, the thresholds and the prox are unchanged.
 *     beta_1 = 0, so Nit <= 2 is exactly the plain iteration.  Every path takes it (row-split,
 *     generic, lrs_ista_pat_f32); the dictionary-resident kernels do not, so a call with accel at
 *     their sizes (n_pad <= 64 with K = 256) runs the row-split kernel and needs its workspace
 *     (lrs_ista_workspace with the same opts).  With warm_start = 1 the call starts from coefs with
 *     the momentum reset (t = 1, x_prev = x_0): an accelerated run sliced over several calls does
 *     NOT reproduce a single call, unlike the plain iteration.  Any other value: LRS_E_INVALID. */
#define LRS_ISTA_F32 0
#define LRS_ISTA_SPLIT_BF16 1
#define LRS_ISTA_ALGO_AUTO 0
#define LRS_ISTA_ALGO_GENERIC 1
#define LRS_ISTA_ACCEL_NONE 0
#define LRS_ISTA_ACCEL_FISTA 1
typedef struct {
    int32_t precision;
    int32_t max_workgroups;
    int32_t algorithm;    /* LRS_ISTA_ALGO_AUTO: the fused kernels for K <= 512, the generic path above;
                             LRS_ISTA_ALGO_GENERIC: every inner iteration as two dense fp32-accurate
                             GEMMs + the prox kernel, chunks of 4096 blocks (any K <= 16384) */
    int32_t warm_start;   /* 1: start from x0 = coefs (on input) instead of 0 and write the result back to
                             coefs, so Nit iterations split over several calls give exactly the
                             iterates of one call (the time-sliced sparse coding beside the DIP, see
                             DESIGN.md §5).  Row-split kernel only (n_pad > 64 or K != 256, or any
                             K <= 512 with accel): LRS_E_UNSUPPORTED elsewhere or without coefs.
                             With accel the momentum restarts in every call (see above). */
    int32_t accel;        /* LRS_ISTA_ACCEL_NONE (0) or LRS_ISTA_ACCEL_FISTA (the first word that was
                             reserved: callers that zeroed it run the plain iteration) */
    int32_t reserved[3];
} lrs_ista_opts;
size_t lrs_ista_workspace(int64_t n, int64_t K, int prox, const lrs_ista_opts *opts);
int lrs_ista_f32(const float *Yb, const uint8_t *obs, const float *D, int64_t n, int64_t n_pad,
                 int64_t K, int64_t nb, const float *alpha, const double *thr, int Nit, int prox,
                 float *coefs, float *phi, const lrs_ista_opts *opts, void *ws, size_t ws_bytes,
                 void *stream);
/* ---- Masked ISTA on per-pattern Grams --------------------------------------------------------
 * The same sparse coding as lrs_ista_f32 for blocks that share observation patterns.  ista()'s
 * gradient H^T (y - H x) (main_LRS_PnP.py:131-149, …1-LiP.py:185-198, H = D pruned to the observed
 * rows by delete_element :201-204) is expanded as b - Q_p x with Q_p = D^T diag(obs_pat[p]) D
 * (fp64 sums of exact products, rounded to float32; formed once per call and pattern) and
 * b = D^T (obs .* y) (once per block), so an inner iteration costs 2 K^2 instead of 4 n K FLOP per
 * block.  Products on f32 matrix cores, the prox and the quotient as lrs_ista_f32: the results
 * differ from it by rounding only.  K <= 512, any n (n_pad % 16 == 0), every prox; opts as
 * lrs_ista_f32 (max_workgroups bounds the grid over tiles, warm_start continues from coefs;
 * algorithm must be AUTO).
 *   lrs_ista_pat_plan (host): groups the blocks by pattern.  pat: host int32 [nb], block j's row of
 *     obs_pat (as lrs_ista_alpha_f32's patterns); plan: host int32 [cap >= lrs_ista_pat_plan_len]
 *     = the blocks ordered by pattern (ascending within one), then per tile {first position,
 *     pattern * 32 + count (1..16)}.  Returns the tile count (< 0: error).  Upload it as is.
 *   lrs_ista_pat_preferred (host): 1 when this path does less matrix-core work than lrs_ista_f32's
 *     row-split kernel for these sizes (few patterns, n > K / 2).
 *   lrs_ista_pat_prepare: forms the dictionary images and every pattern's Q_p in ws
 *     (lrs_ista_pat_workspace bytes), once per D and set of patterns (both fixed for a solve);
 *     obs_pat DEVICE u8 [npat][n_pad].
 *   lrs_ista_pat_f32: the sparse coding on the images ws holds (prepare first, again whenever D or
 *     obs_pat change); plan DEVICE int32 (lrs_ista_pat_plan's); Yb [nb][n_pad], alpha/thr [nb] per
 *     block. */
int64_t lrs_ista_pat_plan_len(int64_t nb, int64_t npat);
int64_t lrs_ista_pat_plan(const int32_t *pat, int64_t nb, int64_t npat, int32_t *plan, int64_t cap);
int lrs_ista_pat_preferred(int64_t n, int64_t K, int64_t nb, int64_t npat, int Nit);
size_t lrs_ista_pat_workspace(int64_t n, int64_t K, int64_t npat);
int lrs_ista_pat_prepare(const float *D, int64_t n, int64_t K, const uint8_t *obs_pat, int64_t npat,
                         int64_t n_pad, void *ws, size_t ws_bytes, void *stream);
int lrs_ista_pat_f32(const float *Yb, const uint8_t *obs_pat, int64_t npat, const int32_t *plan,
                     int64_t ntiles, int64_t n, int64_t n_pad, int64_t K, int64_t nb,
                     const float *alpha, const double *thr, int Nit, int prox, float *coefs, float *phi,
                     const lrs_ista_opts *opts, void *ws, size_t ws_bytes, void *stream);
/* ---- Dictionary learning: the dictionary step of masked alternating minimisation -------------
 * The reference loads its dictionary from trained_dictionary.mat (main_LRS_PnP.py:159-160, variable
 * Dictionary), whose training code was never published.  These calls learn it from the observed
 * blocks: with the coefficients A = coefs fixed (a sparse-coding pass of lrs_ista_f32 /
 * lrs_ista_pat_f32 with LRS_PROX_SOFT), n_inner majorisation-minimisation iterations (Yaghoobi,
 * Blumensath, Davies) of
 *   min_D  sum_j 1/2 ||obs_j .* (y_j - D a_j)||^2   subject to ||d_k||_2 <= 1:
 *   R = obs .* (Yb - coefs D^T);  obj = 1/2 ||R||_F^2;  G = R^T coefs;
 *   u_k = d_k + g_k / c;  d_k = u_k / max(1, ||u_k||_2)
 * with c >= lambda_max(coefs^T coefs), so obj cannot rise.  Layouts are the ISTA calls': Yb, obs
 * [nb][n_pad] (columns >= n never contribute), coefs [nb][K], D n x K row-major.  The three products
 * run on the bf16 matrix cores (three-term split, fp32-GEMM accuracy); obj and the column norms are
 * fp64; every sum runs in a fixed order (bit-identical reruns).  K <= 512, nb <= 2^24
 * (LRS_E_UNSUPPORTED above), n_pad % 16 == 0.
 *   lrs_dict_workspace: bytes of `ws` for both calls below at these sizes (0: bad sizes).
 *   lrs_dict_stats_f32: H = coefs^T coefs (K x K float32) and *c = max_k sum_l |H_kl| (device
 *     double, fp64 sums over the stored H: Gershgorin's bound on lambda_max).
 *   lrs_dict_update_f32: n_inner iterations in place on D.  c: device double (read on the device;
 *     c = 0, every coefficient zero, leaves D as it is); an atom no block uses (H_kk = 0) gets
 *     g_k = 0.  obj: n_inner + 1 device doubles, the objective before each iteration and after the last.
 *   lrs_dict_normalise_f32: every column of D with a non-zero norm scaled to unit norm
 *     (columnNormalise.m), the last step of a training run. */
size_t lrs_dict_workspace(int64_t n, int64_t n_pad, int64_t K, int64_t nb);
int lrs_dict_stats_f32(const float *coefs, int64_t nb, int64_t K, float *H, double *c, void *ws,
                       size_t ws_bytes, void *stream);
int lrs_dict_update_f32(const float *Yb, const uint8_t *obs, const float *coefs, float *D, int64_t n,
                        int64_t n_pad, int64_t K, int64_t nb, const double *c, int n_inner, double *obj,
                        void *ws, size_t ws_bytes, void *stream);
int lrs_dict_normalise_f32(float *D, int64_t n, int64_t K, void *stream);
/* NLmeansfilter(g, 3, 3, h) (LRS-PnP(Matlab Code)/NLmeansfilter.m:18-78, the prox of
 * pnp_ista.m:30) of nvec columns of length K, fp64, 'symmetric' padding. */
int lrs_nlm_matlab_col_f32(const float *g, int64_t ldg, float *out, int64_t ldo, int64_t K,
                           int64_t nvec, double h, const double *h_per_vec, void *stream);
/* Options of the DIP engine and the conv primitives (NULL = defaults), fixed per call or, for a
 * lrs_dipnet, at creation -- the library keeps no process-wide mode:
 *   precision: arithmetic of the conv GEMMs.  LRS_DIP_SPLIT_BF16 (default): bf16 matrix cores on
 *     operands split into three bf16 terms, six partial products, fp32 accumulation (fp32-GEMM
 *     accuracy); LRS_DIP_F32: v_mfma_f32_16x16x4_f32 (the explicit-im2col kernels; a lrs_dipnet
 *     created with it runs every conv on them).
 *   upsample_dgrad: data gradient of an upsampled stride-1 conv (nearest x2, then 2x2 unpadded or
 *     3x3 pad 1): 0 (default) = correlation over the padded upsampled domain + fold; 1 = a stride-2
 *     conv with the (k+1)x(k+1) effective kernel on the source grid (2.25x fewer products) +
 *     reflection border terms.  lrs_conv2d_workspace must be queried with the same options. */
#define LRS_DIP_F32 0
#define LRS_DIP_SPLIT_BF16 1
typedef struct {
    int32_t precision;
    int32_t upsample_dgrad;
    int32_t reserved[6];
} lrs_dip_opts;

/* ---- SVT low-rank prox ---------------------------------------------------------------------
 * U = SVT(Z, tau) with Z = X + c2 * L2 (c2 = float(1/mu_2); L2 may be NULL), via an fp64 Gram
 * Z^T Z, a one-workgroup symmetric eigensolver and U = Z * V diag(max(1 - tau/s, 0)) V^T.
 * `warm` is a flag word:
 *   default (0): Householder tridiagonalisation + multisection + inverse iteration with a
 *     Davis-Kahan orthogonality certificate, falling back (inside the same workgroup) to the
 *     Jacobi solve when the certificate fails (clustered / repeated eigenvalues);
 *   LRS_SVT_JACOBI: the cyclic Jacobi solver only, warm-started from the previous call's
 *     eigenvectors kept in ws when LRS_SVT_WARM is also set;
 *   LRS_SVT_MULTI_WG (default path only): the same solver with its eigenvalue, inverse-iteration
 *     and back-transformation phases spread over many workgroups (bit-identical result); for a
 *     caller whose eigensolver is on the critical path (a row-slab shard), not beside a
 *     chip-filling sparse-coding kernel.
 * s_out (nullable, device, B doubles) receives the singular values (descending).  Up to 198 bands
 * the eigensolver holds the packed fp64 Gram in its CU's LDS, above it (the 224-band cubes) the
 * same one-workgroup chain works on the packed Gram in ws (L2-resident), up to 256 bands.
 * Wide cubes, 256 < B <= lrs_svt_max_bands() = 512: the Gram and U = Z (I - E) are tiled over
 * column panels, and the eigen stage is by default the one-workgroup Jacobi chain, whatever the
 * LRS_SVT_JACOBI bit says (the state word reports path 3).  LRS_SVT_WARM alone enables its warm
 * start there: _gram then forms the warm-start products V^T (G V).  LRS_SVT_MULTI_WG with
 * B > 256 is LRS_E_UNSUPPORTED, as is any B above 512 (main_LRS_PnP.py:112-124's np.linalg.svd
 * takes any B).  The workspace grows with the rotation log: 131 MB at (P, B) = (40000, 512).
 *   LRS_SVT_WIDE_TRI (256 < B <= 512; ignored below, where the calls launch what they launch
 *     without it): the tridiagonal solver instead of the Jacobi chain: a one-workgroup Householder
 *     reduction, then eigenvalues, inverse iteration and back-transformation over many workgroups
 *     and the certificate as fp64 matrix-core GEMMs, falling back to the Jacobi solve of the same
 *     Gram when the certificate fails.  State path 4 (certified) or 5 (fallback).  It needs no
 *     warm start (with LRS_SVT_WARM, _gram skips the products) and leaves its eigenvectors for a
 *     later warm Jacobi call on the same ws.  LRS_SVT_JACOBI set as well: the Jacobi chain.  The
 *     workspace is the same size.
 *   LRS_SVT_WIDE_MW (with LRS_SVT_WIDE_TRI on 256 < B <= 512; ignored wherever that chain does not
 *     serve: B <= 256, LRS_SVT_WIDE_TRI not set, or LRS_SVT_JACOBI set): that chain with its
 *     Householder reduction spread over many workgroups as well, one launch per column of the Gram
 *     (Bp launches on the caller's stream, the launch boundary the only synchronisation between
 *     workgroups; fixed-order sums, so reruns are bit-identical); every later phase is the same.
 *     _gram treats it as LRS_SVT_WIDE_TRI alone.  Diagnostic state word 7 is 1 after such a solve
 *     and 0 after a solve of the one-workgroup reduction; the path is still 4 or 5.  The workspace
 *     is the same size: the reduction's scratch aliases regions that are dead while it runs.
 * What ws holds before a call: a cold call of a wide cube (256 < B <= 512; the flag word 0,
 * LRS_SVT_WIDE_TRI, or LRS_SVT_WIDE_TRI | LRS_SVT_WIDE_MW) ignores the workspace's contents.  It
 * clears the state words itself and reads nothing past them that it has not written in the same
 * call, so it needs no zeroed workspace and gives the same bits after any earlier call of any chain
 * on that ws.  Only a call with LRS_SVT_WARM reads what the call before it left (the state words
 * and the eigenvectors), and needs the first 256 bytes of a new ws to be zero. */
#define LRS_SVT_WARM 1
#define LRS_SVT_JACOBI 2
#define LRS_SVT_MULTI_WG 4
#define LRS_SVT_WIDE_TRI 8
#define LRS_SVT_WIDE_MW 16
/* The largest band count the SVT calls accept (host-only): 512. */
int64_t lrs_svt_max_bands(void);
size_t lrs_svt_workspace(int64_t P, int64_t B);
int lrs_svt_f32(const float *X, const float *L2, float c2, int64_t P, int64_t B, double tau,
                float *U, double *s_out, int warm, void *ws, size_t ws_bytes, void *stream);
/* The same call split in two stream-ordered halves so the caller can start the sparse-coding
 * kernel between them: _gram (multi-workgroup Gram, plus the warm-start products for
 * LRS_SVT_JACOBI | LRS_SVT_WARM) and _finish (the one-workgroup eigensolver, then U), which then
 * runs beside the sparse coding. */
int lrs_svt_gram_f32(const float *X, const float *L2, float c2, int64_t P, int64_t B, int warm,
                     void *ws, size_t ws_bytes, void *stream);
int lrs_svt_finish_f32(const float *X, const float *L2, float c2, int64_t P, int64_t B, double tau,
                       float *U, double *s_out, int warm, void *ws, size_t ws_bytes, void *stream);
/* Byte offset and leading dimension (Bp = B rounded up to even) of the fp64 Gram (X + c2 L2)^T
 * (X + c2 L2) that lrs_svt_gram_f32 leaves in ws. A caller that holds one row slab of the
 * unfolded cube per rank sums the slabs' Grams in place (all-reduce of Bp*Bp doubles) between
 * _gram and _finish: the Gram is additive over pixel rows (single cube on
 * several GPUs). Not valid with LRS_SVT_JACOBI | LRS_SVT_WARM (its warm-start products are
 * formed from the local Gram inside _gram), nor for the wide cubes above 256 bands, whose eigen
 * stage is that path: LRS_E_UNSUPPORTED there. Host-only, no device access. */
int lrs_svt_gram_offset(int64_t P, int64_t B, int64_t *offset_bytes, int64_t *ld);

/* ---- TV prox on the cube: a learning-free choice for the low-rank slot -----------------------
 * An extension (the reference's U update is the SVT or a DIP; admm_utils.py carries a tv_prox it never
 * calls).  X, L2, U are [P][B] as for the SVT, P = H W, p = i + H j, and the image is
 * o[c = b][y = i][x = j] (lrs_unfolded_to_image_f32's map).  With Z = fl(X + fl(c2 L2)) (L2 nullable):
 *   U = argmin_u 1/2 ||u - Z||^2 + tau T(u)
 *   T(u) = w_sp sum(|Dy u| + |Dx u|) + w_bd sum |Dc u| + w_ss sum(|Dy Dc u| + |Dx Dc u|),
 * the operators, their association and their index sets those of lrs_sstv_f32 below: T(u) is N R of that
 * call with eps = 0.  Any H, W, B with H W B < 2^31 (LRS_E_UNSUPPORTED from there on).
 * The algorithm is fixed: n_iter iterations of the fast gradient projection on the dual (Beck-Teboulle
 * FGP) in fp32.  K stacks the operators whose weight is > 0, the box radii are r = (float)(tau w), the step
 * is the fp32 1 / L, L = 8 [w_sp > 0] + 4 [w_bd > 0] + 32 [w_ss > 0] >= ||K||^2:
 *   p = 0, q = p, t = 1;  n_iter times:  u = Z - K^T q;  p_new = clip(q + (1/L) K u, -r, r);
 *   t_new = (1 + sqrt(1 + 4 t^2)) / 2, beta = (float)((t - 1) / t_new) (fp64 on the host, as
 *   LRS_ISTA_ACCEL_FISTA);  q = p_new + beta (p_new - p);  then U = Z - K^T p.
 * K^T is a gather in a fixed order without float atomics: reruns are bit-identical, and so are calls whose
 * bases are aligned differently.  Two launches per iteration on the caller's stream; the call never
 * allocates and never synchronises, and every refusal is decided on the host before a launch.
 * stats (nullable, device, 2 doubles): the primal objective 1/2 ||U - Z||^2 + tau T(U) and the duality gap
 * sum_f r_f |K_f U| - <p, K U> of the returned pair, as fp64 sums in a fixed order: how a caller chooses
 * n_iter.  All weights 0, tau = 0 or n_iter = 0: U = Z by one copy kernel, and stats is the pair (Z, p = 0)'s,
 * {tau T(Z), tau T(Z)} -- {0, 0} unless only n_iter is 0.
 * flags: LRS_TVPROX_WARM starts from the p the previous call left in the same ws, clipped to this call's
 * radii, with the momentum reset (t = 1).  The caller guarantees that that call had the same (H, W, B) and
 * the same set of weights > 0, and ran at least one iteration; without the flag the contents of ws are
 * ignored.  ws: lrs_tvprox_workspace bytes (for all five fields whatever the weights; 0: a size <= 0 or
 * H W B >= 2^31), 16-byte aligned for the vector forms.  U may alias neither X nor L2.
 * LRS_E_INVALID: X, U or ws NULL, a size <= 0, a negative or NaN weight or tau, n_iter < 0, unknown flag
 * bits.  LRS_E_WORKSPACE: ws_bytes too small. */
#define LRS_TVPROX_WARM 1
size_t lrs_tvprox_workspace(int64_t H, int64_t W, int64_t B);
int lrs_tvprox_f32(const float *X, const float *L2, float c2, int64_t H, int64_t W, int64_t B, float w_sp,
                   float w_bd, float w_ss, double tau, int n_iter, int flags, float *U, double *stats, void *ws,
                   size_t ws_bytes, void *stream);

/* ---- Spectral non-local-means prox on the cube: a fourth choice for the low-rank slot --------
 * An extension (the reference's U update is the SVT or a DIP): the operator of the nlm_prox that
 * admm_utils.py:95-100 carries beside its tv_prox and never calls, denoise_nl_means(img_HWC,
 * multichannel=True, sigma, patch_distance=2, h=0.05), as DEFINED here (not bit parity with skimage): one
 * weight per pixel pair, computed from all bands and applied to every band.
 * X, L2, U are [P][B] as for the TV prox, P = H W, p = y + H x, the image z[c][y][x];
 * Z = fl(X + fl(c2 L2)) (L2 nullable: Z = X).  rp = patch_size / 2 with patch_size odd in {1, 3, 5, 7},
 * rs = patch_distance in 0..5; the host rounds ih2 = (float)(1 / (h h)) and s2 = (float)(2 sigma sigma) once.
 *   m(e), the index an integer e reads on an axis of length n: 0 when n = 1; else with r = e mod 2 (n - 1)
 *     (non-negative), r when r < n and 2 (n - 1) - r otherwise: reflection without repeating the edge, continued
 *     periodically, so defined for every size, those below the pads included
 *   d(e, e') = sum_c (z[c, m(e)] - z[c, m(e')])^2            over 2-D extended coordinates
 *   D(p, t)  = sum_{|dy|, |dx| <= rp} d(p + delta, p + delta + t)
 *   w(p, t)  = exp(-max(D(p, t) / (B (2 rp + 1)^2) - s2, 0) ih2)    so w(p, 0) = 1 exactly
 *   U[c, p]  = sum_t w(p, t) z[c, p + t] / sum_t w(p, t)
 * over the offsets t with |ty|, |tx| <= rs whose candidate p + t lies inside the image (the search window is
 * clipped, not reflected; t = 0 always counts, so the denominator is >= 1).
 * d is summed in fp32 over the bands in ascending order, D and the weight are formed in fp64 and the weight
 * is rounded once to fp32, and both sums over t run in fp64 in a fixed order (ty outer, tx inner) without
 * float atomics: reruns are bit-identical, and so are calls whose bases are aligned differently.
 * One launch on the caller's stream; the call never allocates and never synchronises, and every refusal is
 * decided on the host before the launch (the pointers are not read).  ws: lrs_nlmcube_workspace bytes, which
 * is 0 (the one launch keeps everything in LDS), so ws may be NULL.  U may alias neither X nor L2.
 * LRS_E_INVALID: X or U NULL, ws NULL while the workspace is > 0, a size <= 0, patch_size even or < 1,
 * patch_distance < 0, h <= 0, NaN or inf, sigma < 0 or NaN.  LRS_E_UNSUPPORTED: patch_size > 7,
 * patch_distance > 5, H W B >= 2^31.  LRS_E_WORKSPACE: ws_bytes too small.  An invalid argument wins. */
size_t lrs_nlmcube_workspace(int64_t H, int64_t W, int64_t B, int patch_size, int patch_distance);
int lrs_nlmcube_f32(const float *X, const float *L2, float c2, int64_t H, int64_t W, int64_t B,
                    int patch_size, int patch_distance, double h, double sigma,
                    float *U, void *ws, size_t ws_bytes, void *stream);

/* ---- col2im + closed-form X update + dual updates ------------------------------------------
 * IMout = sum over covering blocks (block order) of phi, Weight = count, lambda1_sum = repeated
 * sum of lambda_1, then (float32, the reference's operation order)
 *   X  = (g*Y + mu1*IMout + mu2*U - lambda1_sum - L2) / (g*M + mu1*Weight + mu2)
 *   L1 = L1 + mu1*(X - IMout);   L2 = L2 + mu2*(X - U)
 * X, L1, L2 updated in place.  rlo/rhi [P], clo/chi [B]: device cover ranges over the sorted
 * block-row / block-column starts (lrs_cover_ranges); nbr = number of block rows.
 * norms (nullable, device, 3 doubles, zeroed by the call) += ||dX||^2, ||dL1||^2, ||dL2||^2.
 * imout (nullable) receives IMout. */
int lrs_admm_update_f32(float *X, float *L1, float *L2, const float *Y, const float *M,
                        const float *U, const float *phi, int64_t P, int64_t B, int64_t bb,
                        int64_t n_pad, const int32_t *row_starts, const int32_t *col_starts,
                        int64_t nbr, const int32_t *rlo, const int32_t *rhi, const int32_t *clo,
                        const int32_t *chi, float gamma, float mu1, float mu2, double *norms,
                        float *imout, void *stream);

/* ==== DIP low-rank prox (the 1-Lipschitz U-Net of main_LRS_PnP_DIP_1-LiP.py) ================
 * Activations are [C][H][W] float32 (batch 1).  Reference interfaces replaced:
 *   lrs_conv2d_*        ReflectionPad2d + Conv2d + nn.Upsample(x2, nearest)
 *                       (models/lipschitz_constraint_layer.py:65-78, my_Lipschitz_Unet.py:71-94)
 *   lrs_bn_act_*        BatchNormSpectralNorm-wrapped BatchNorm2d (train mode) + LeakyReLU(0.2)
 *                       (lipschitz_constraint_layer.py:88-122,154-159, 6-22)
 *   lrs_sigma_max_f32   SpectralNorm._update_u_v: torch.svd(W.view(Co,-1))[0]  (:36-44)
 *   lrs_adam_f32        torch.optim.Adam(lr) step                      (…1-LiP.py:215,237)
 *   lrs_masked_mse_f32  MSELoss(target*mask, out*mask) + its gradient  (…1-LiP.py:216,234);
 *                       _cmask: the same under a per-band mask [C][P]
 *   lrs_es_*            EarlyStop / myMetric variance test             (…1-LiP.py:71-103,244-264)
 *   lrs_dipnet_*        my_Lipschitz_Unet + the get_DIP_out training loop (…1-LiP.py:208-264) */
#define LRS_PAD_ZERO 0
#define LRS_PAD_REFLECT 1
#define LRS_ACT_NONE 0
#define LRS_ACT_LRELU 1   /* LeakyReLU(0.2) */
#define LRS_ACT_SIGMOID 2
#define LRS_ACT_RELU 3    /* ReLU: LRS_NODE_DECODE and lrs_up2_bilinear_act_* only (LRS_E_INVALID elsewhere) */

/* Output size of the conv unit (upsample, pad, k, stride). */
int lrs_conv2d_out_size(int H, int W, int k, int stride, int pad, int upsample, int *Ho, int *Wo);
/* col workspace (floats) for lrs_conv2d_fwd_f32: Cin*k*k*Ho*Wo (0 when the unit is a plain 1x1). */
int64_t lrs_conv2d_col_size(int Cin, int H, int W, int k, int stride, int pad, int upsample);
/* y[Cout][Ho][Wo] = conv(pad(upsample(x))) + bias.  col receives the im2col matrix (kept for
 * the backward); col == NULL (k <= 3): implicit GEMM, the im2col is gathered inside the
 * split-bf16 kernel and never stored (backward: lrs_conv2d_bwd_x_f32).
 * ws/ws_bytes: split-K partials (lrs_conv2d_workspace). */
size_t lrs_conv2d_workspace(int Cin, int H, int W, int Cout, int k, int stride, int pad, int upsample,
                            const lrs_dip_opts *opts);
int lrs_conv2d_fwd_f32(const float *x, int Cin, int H, int W, const float *w, const float *bias,
                       int Cout, int k, int stride, int pad, int pad_mode, int upsample, float *col,
                       float *y, const lrs_dip_opts *opts, void *ws, size_t ws_bytes, void *stream);
/* gw = (gy col^T) / *w_div (w_div nullable, device scalar: the spectral-norm scale);
 * gx (nullable) = adjoint of the im2col of gy through w.  gbias is produced by lrs_bn_act_bwd.
 * col = the forward's col (or x itself for a plain 1x1 unit). */
int lrs_conv2d_bwd_f32(const float *gy, const float *col, const float *w, const float *w_div, int Cin,
                       int H, int W, int Cout, int k, int stride, int pad, int pad_mode, int upsample,
                       float *gx, float *gw, const lrs_dip_opts *opts, void *ws, size_t ws_bytes,
                       void *stream);
/* The same from the conv input x (k <= 3): gw's col^T is gathered inside the GEMM. */
int lrs_conv2d_bwd_x_f32(const float *gy, const float *x, const float *w, const float *w_div, int Cin,
                         int H, int W, int Cout, int k, int stride, int pad, int pad_mode, int upsample,
                         float *gx, float *gw, const lrs_dip_opts *opts, void *ws, size_t ws_bytes,
                         void *stream);

/* y = act(BN_lip(z)) with batch statistics (gamma == NULL: y = act(z)).  Saves mean / invstd
 * [C]; running stats (nullable) get the momentum update.  ws: lrs_bn_act_workspace bytes,
 * zero-filled before its first use (it is left zeroed for the next call). */
size_t lrs_bn_act_workspace(int C, int64_t P);
int lrs_bn_act_fwd_f32(const float *z, float *y, const float *gamma, const float *beta, float *mean,
                       float *invstd, float *run_mean, float *run_var, int C, int64_t P, int act,
                       float eps, float momentum, void *ws, size_t ws_bytes, void *stream);
int lrs_bn_act_bwd_f32(const float *gy, const float *y, const float *z, const float *gamma,
                       const float *mean, const float *invstd, float *gz, float *ggamma,
                       float *gbeta, float *gbias, int C, int64_t P, int act, void *ws, size_t ws_bytes,
                       void *stream);
/* Conv -> BatchNorm(train) -> act in one launch on a small map (the network engine's forward for the
 * <= 9^2 maps): z = conv(reflect_pad(x)) + bias (bias nullable), y = act(BN_lip(z)), mean / invstd
 * [Cout] saved, running stats (nullable, both or neither) momentum-updated (eps 1e-5, momentum 0.1);
 * lip = 1: BatchNormSpectralNorm's gamma / c, beta / c.  Replaces a Conv2d + BatchNorm2d +
 * LeakyReLU block (lipschitz_constraint_layer.py:65-78,88-101, models/common.py:71-121).
 * LRS_E_UNSUPPORTED where the one-launch kernel does not take the geometry (zero padding, upsample,
 * a source under 2 x 2, > 1024 output pixels, more than two staged input chunks). */
int lrs_conv_bn_small_f32(const float *x, int Cin, int H, int W, const float *w, const float *bias, int Cout,
                          int k, int stride, int pad, int pad_mode, int upsample, const float *gamma,
                          const float *beta, int lip, int act, float *z, float *y, float *mean, float *invstd,
                          float *run_mean, float *run_var, void *stream);
/* Bilinear x2 upsampling fused with an activation, the two kernels of a Deep Decoder stage
 * (LRS_NODE_DECODE; include/decoder.py decodernw: nn.Upsample(scale_factor=2, mode='bilinear'), then
 * act_fun).  x is [C][H][W], y and gy are [C][2H][2W].  align_corners=False: per axis output 2s + p takes
 * 3/4 of source s and 1/4 of s - 1 (p = 0) or s + 1 (p = 1), that index clamped at both edges.
 *   _fwd: y = act(up2(x)).
 *   _bwd: gx = up2^T(gy .* act'(y)), a gather in a fixed order (no atomics: reruns are bit-identical);
 *         act' is taken from the sign of the stored y (y = 0: the slope of x <= 0, as torch).
 * act: LRS_ACT_NONE, LRS_ACT_LRELU or LRS_ACT_RELU (LRS_E_INVALID otherwise); C <= 65535 and
 * 4 H W < 2^31 (LRS_E_UNSUPPORTED above). */
int lrs_up2_bilinear_act_fwd_f32(const float *x, int C, int H, int W, int act, float *y, void *stream);
int lrs_up2_bilinear_act_bwd_f32(const float *gy, const float *y, int C, int H, int W, int act, float *gx,
                                 void *stream);

/* sigma_max of n weight matrices W[i] (rows[i] x cols[i], min(rows, cols) <= 128; host arrays
 * of device pointers), within 1 float32 ulp of the fp64 SVD value for 5e-20 < sigma < 1e19, unless the
 * top singular vector's component along the Lanczos start vector is below c(g) for the relative gap g
 * to sigma_2 (3e-8 at g = 1e-3 ... 3e-4 at g = 1e-6, csrc/dip_sn.h); sigma is then low by at most the
 * gap, never high.  scale = max(1, sigma/ln_lambda) and, when Wn != NULL, Wn[i] = W[i] / scale[i]. */
size_t lrs_sigma_max_workspace(int n);
int lrs_sigma_max_f32(const float *const *W, float *const *Wn, const int *rows, const int *cols, int n,
                      float ln_lambda, float *sigma, float *scale, void *ws, size_t ws_bytes,
                      void *stream);

/* One Adam step over a flat buffer; step (device int) is the 1-based step count. */
int lrs_adam_f32(float *p, const float *g, float *m, float *v, int64_t n, const int *step, float lr,
                 float beta1, float beta2, float eps, void *stream);
/* loss_acc (device double) += sum((target*mask - out*mask)^2); gout (nullable) = dL/dout of the
 * mean.  mask (nullable) is [P], broadcast over the C channels. */
int lrs_masked_mse_f32(const float *out, const float *target, const float *mask, int C, int64_t P,
                       float *gout, double *loss_acc, void *stream);
/* The same with a mask of mask_channels channels: 1 = [P] (lrs_masked_mse_f32 is this case), C =
 * per element [C][P], the layout of out and target: a mask that differs between bands (dead
 * columns, dropped lines, missing bands).  Generalises …1-LiP.py:234, whose mask_bkg is
 * (1,1,H,W); the mean stays over all C*P elements.  Any other count: LRS_E_INVALID. */
int lrs_masked_mse_cmask_f32(const float *out, const float *target, const float *mask, int mask_channels,
                             int C, int64_t P, float *gout, double *loss_acc, void *stream);
/* The same for an output that holds its image inside a frame (lrs_dipnet_set_frame): the mask is 0 on
 * the frame, so the sum runs over the image alone and gout is 0 on the frame; gout = dL/dout of the mean
 * over n_mean elements (the image's C*H*W, 0 < n_mean <= C*P) instead of C*P.  n_mean = C*P is
 * lrs_masked_mse_cmask_f32, launch for launch. */
int lrs_masked_mse_framed_f32(const float *out, const float *target, const float *mask, int mask_channels,
                              int C, int64_t P, int64_t n_mean, float *gout, double *loss_acc, void *stream);
/* Smoothness term on the net's output, an extension (the reference's loss is the masked MSE alone;
 * admm_utils.py carries a tv_prox it never calls): anisotropic spatial TV, band TV and spatial-spectral TV
 * (SSTV) of the image o = the H x W pixels at (top, left) of out[C][Hf][Wf].  With N = n_mean and
 * phi(d) = sqrt(d^2 + eps^2) (|d| for eps = 0):
 *   R(o) = (w_sp / N) sum [ phi(o[c,y+1,x] - o[c,y,x]) + phi(o[c,y,x+1] - o[c,y,x]) ]
 *        + (w_bd / N) sum   phi(o[c+1,y,x] - o[c,y,x])
 *        + (w_ss / N) sum [ phi(Dy Dc o) + phi(Dx Dc o) ],
 *   Dy Dc o[c,y,x] = (o[c+1,y+1,x] - o[c,y+1,x]) - (o[c+1,y,x] - o[c,y,x]), Dx Dc likewise along x,
 * each sum over the indices whose operands all lie inside the image (empty for C, H or W = 1): nothing is
 * padded, and nothing of the frame is used.  gout (nullable, the layout of out) += dR/do on the image, its
 * frame untouched, with phi'(d) = d / sqrt(d^2 + eps^2), for eps = 0 sign(d) with sign(0) = 0; a gather in a
 * fixed order (no atomics: reruns are bit-identical).  loss_acc (nullable, device double) += N R, so that
 * after lrs_masked_mse_framed_f32 on the same gout and accumulator, gout is dL/dout of masked MSE + R --
 * what lrs_dipnet_backward takes -- and loss_acc / N that loss.  (lrs_dipnet_train_steps* train on the masked
 * MSE alone.)
 * LRS_E_INVALID: out NULL, a size <= 0, an image that does not fit the frame, a negative weight or eps,
 * n_mean <= 0.  All three weights 0: LRS_OK, nothing is launched. */
int lrs_sstv_f32(const float *out, int C, int Hf, int Wf, int top, int left, int H, int W, float w_sp, float w_bd,
                 float w_ss, float eps, int64_t n_mean, float *gout, double *loss_acc, void *stream);

/* Layout transforms between the unfolded matrix X[p = i + H j][b] and the DIP image img[b][i][j]
 * (…1-LiP.py:404 DIP_input = X + (1/mu_2) lambda_2 as (1,B,H,W); :411 U back to (P,B)). */
int lrs_unfolded_to_image_f32(const float *X, const float *L, float c, int64_t H, int64_t W, int64_t B,
                              float *img, void *stream);
int lrs_image_to_unfolded_f32(const float *img, int64_t H, int64_t W, int64_t B, float *X, void *stream);
/* The same two for an image held inside a frame: img is [B][Hf][Wf] with the H x W image at rows
 * top.., columns left...  _to_frame also fills the frame by reflection without repeating the edge
 * (nn.ReflectionPad2d((left, Wf-W-left, top, Hf-H-top)) of the image), in the one pass that reads the
 * unfolded rows; _frame_to_unfolded reads the interior only.  Every pad must be smaller than the
 * dimension it mirrors (ReflectionPad2d's own rule): LRS_E_INVALID otherwise.  An extension: the
 * reference has no frame (its net refuses the sizes that need one). */
int lrs_unfolded_to_frame_f32(const float *X, const float *L, float c, int64_t H, int64_t W, int64_t B,
                              int64_t top, int64_t left, int64_t Hf, int64_t Wf, float *img, void *stream);
int lrs_frame_to_unfolded_f32(const float *img, int64_t H, int64_t W, int64_t B, int64_t top, int64_t left,
                              int64_t Hf, int64_t Wf, float *X, void *stream);

/* Early stopping state (device memory).  lrs_es_init fills it; every lrs_es_update_f32 pushes one
 * output into the ring and, once full, applies the variance test.  ring: lrs_es_ring_bytes(size, N)
 * bytes of device memory -- the last `size` outputs as [size][N] floats (slot = epoch % size), then
 * the per-pixel window sums (fp64) and the window's sum of squares that the test slides from step to
 * step. */
typedef struct {
    int32_t count, size, patience, wait, stop, stop_epoch, best_epoch, reserved;
    double best, var_acc, last_var;   /* var_acc: unused (lrs_es_init zeroes it); kept for the layout */
} lrs_es_state;
size_t lrs_es_ring_bytes(int size, int64_t N);
int lrs_es_init(lrs_es_state *st, int size, int patience, void *stream);
int lrs_es_update_f32(const float *out, int64_t N, float *ring, lrs_es_state *st, void *stream);

/* ---- Whole network + training step ---------------------------------------------------------
 * A DAG of nodes; tensor 0 is the network input (C x H x W), node i produces tensor i + 1 and
 * may read any earlier tensor.  The 1-Lip U-Net is a chain of CONV nodes; the skip net
 * (models/skip.py) adds BN and CONCAT nodes.  The host object holds shapes and offsets only;
 * parameters, gradients, Adam moments and the workspace are caller-owned device buffers given
 * to lrs_dipnet_bind. */
#define LRS_NODE_CONV 0    /* [upsample x2] -> pad -> conv(k, stride) -> [BN] -> act            */
#define LRS_NODE_BN 1      /* BN -> act on in0                                                  */
#define LRS_NODE_CONCAT 2  /* cat(in0, [upsample x2](in1)) along channels, centre-cropped       */
/* One Deep Decoder stage on in0 (include/decoder.py decodernw, bn_before_act=False):
 *   conv 1x1 to cout channels, no bias -> [bilinear x2] -> act -> [BN]
 * -- the activation comes BEFORE the BatchNorm.  Fields used: cout, upsample (0 or LRS_UP_BILINEAR), act,
 * bn (LRS_BN_NONE or LRS_BN_PLAIN), winit.  k must be 1, stride 1, pad 0, sn 0, upsample not nearest and
 * bn not LRS_BN_LIP: LRS_E_UNSUPPORTED from lrs_dipnet_create otherwise.  act: NONE, LRELU, RELU, or
 * SIGMOID with upsample = 0 and bn = 0 only (the head; LRS_E_INVALID with either).  The node owns a weight
 * [cout][cin] and, with bn, gamma and beta; it has no bias (lrs_dipnet_param_offsets: b = -1).  As the
 * last node, a stage without upsampling and BN takes the loss head a bias-free CONV head would. */
#define LRS_NODE_DECODE 3
/* upsample values: 0 none, 1 nearest (CONV / CONCAT, which take any non-zero value but LRS_UP_BILINEAR as
 * nearest and refuse LRS_UP_BILINEAR with LRS_E_INVALID), 2 bilinear (DECODE only) */
#define LRS_UP_BILINEAR 2
#define LRS_BN_NONE 0
#define LRS_BN_PLAIN 1     /* nn.BatchNorm2d, train mode (models/common.py:71)                 */
#define LRS_BN_LIP 2       /* BatchNormSpectralNorm-wrapped (lipschitz_constraint_layer.py:88)  */
#define LRS_WINIT_DEFAULT 0   /* nn.Conv2d default init: U(-1/sqrt(fan_in), +)                  */
#define LRS_WINIT_KAIMING 1   /* kaiming_uniform_(a=0, fan_in) (lipschitz_constraint_layer.py:74) */
typedef struct {
    int32_t kind, in0, in1, cout, k, stride, pad, pad_mode, upsample, bn, act, sn, winit;
} lrs_dip_node;
typedef struct lrs_dipnet lrs_dipnet;
int lrs_dipnet_create(const lrs_dip_node *nodes, int n_nodes, int C, int H, int W, const lrs_dip_opts *opts,
                      lrs_dipnet **out);
/* the options the net was created with */
int lrs_dipnet_get_opts(const lrs_dipnet *net, lrs_dip_opts *opts);
void lrs_dipnet_destroy(lrs_dipnet *net);
int64_t lrs_dipnet_num_params(const lrs_dipnet *net);
int64_t lrs_dipnet_num_bnstats(const lrs_dipnet *net);
size_t lrs_dipnet_workspace(const lrs_dipnet *net);
/* offsets (floats) of node i's parameters in the flat buffer; -1 when absent */
int lrs_dipnet_param_offsets(const lrs_dipnet *net, int node, int64_t *w, int64_t *b, int64_t *gamma,
                             int64_t *beta);
/* shape of node i's output (node = -1: the input) */
int lrs_dipnet_node_shape(const lrs_dipnet *net, int node, int *C, int *H, int *W);
int lrs_dipnet_out_shape(const lrs_dipnet *net, int *C, int *H, int *W);
int lrs_dipnet_bind(lrs_dipnet *net, float *params, float *grads, float *adam_m, float *adam_v,
                    float *bnstats, void *ws, size_t ws_bytes);
/* Conv weights per node winit, torch-default biases, gamma = 1, beta = 0, zero Adam state; a
 * counter-based RNG keyed by seed (the reference draws from the unseeded torch RNG). */
int lrs_dipnet_init_params(lrs_dipnet *net, uint64_t seed, void *stream);
/* zero the Adam moments and the step count (a fresh optimizer on the current parameters) */
int lrs_dipnet_reset_optimizer(lrs_dipnet *net, void *stream);
/* forward only (spectral norms included); the output stays in lrs_dipnet_output() */
int lrs_dipnet_forward(lrs_dipnet *net, const float *x, void *stream);
/* backward from gout = dL/d(output) (C x H x W, device) through the activations of the last
 * lrs_dipnet_forward on the same x: every parameter gradient into the bound grads buffer (sigma
 * and the BN scale c are constants, as the reference takes them from .data); no input gradient.
 * Replaces loss.backward() through my_Lipschitz_Unet / skip (…1-LiP.py:237, pro :245). */
int lrs_dipnet_backward(lrs_dipnet *net, const float *x, const float *gout, void *stream);
/* ln_lambda of the spectral normalisation (my_Lipschitz_Unet(..., ln_lambda); default 1) */
int lrs_dipnet_set_ln_lambda(lrs_dipnet *net, float ln_lambda);
/* The image inside the net's output: H x W pixels at (top, left) of the Ho x Wo output, for a net
 * trained on an image of a size it does not reproduce, padded to one it does.  The target's and the
 * input's frame contents are the caller's (lrs_unfolded_to_frame_f32); the mask must be 0 on the frame.
 * With a frame set, lrs_dipnet_train_steps* take the loss as the mean over the image's C*H*W elements
 * (gradient and lrs_dipnet_last_loss alike), and es / ring see the image only: ring is sized for
 * N = C*H*W and holds the cropped outputs [C][H][W].  Call it between steps (it is part of the captured
 * graph's key).  The whole output (0, 0, Ho, Wo), the state after lrs_dipnet_create, is no frame: the
 * step then launches exactly the kernels it launches without this call.  Every pad must be smaller
 * than the dimension it mirrors. */
int lrs_dipnet_set_frame(lrs_dipnet *net, int top, int left, int H, int W);
int lrs_dipnet_get_frame(const lrs_dipnet *net, int *top, int *left, int *H, int *W);
const float *lrs_dipnet_output(const lrs_dipnet *net);
const float *lrs_dipnet_grads(const lrs_dipnet *net);
/* diagnostics: node i's buffers in the workspace after a forward / backward (NULL where absent):
 * its output, its pre-BatchNorm z, dL/dz, dL/d(output).  A DECODE stage with BatchNorm: z is the
 * activation a the BatchNorm reads (the node's shape), dL/dz its gradient; a DECODE stage without: as a
 * CONV without BatchNorm where it neither upsamples nor applies ReLU, else NULL for both. */
#define LRS_BUF_OUT 0
#define LRS_BUF_Z 1
#define LRS_BUF_GZ 2
#define LRS_BUF_GRAD 3
const float *lrs_dipnet_node_buffer(const lrs_dipnet *net, int node, int which);
/* nsteps training steps: forward, masked MSE, backward, Adam; es (nullable) gets every step's
 * forward output (ring: es->size * C*H*W floats).  use_graph != 0 captures one step into a
 * hipGraph (on first use, re-captured when any argument changes) and replays it.  The weight
 * gradients run on a second stream the net owns with the calling stream's priority (one such
 * stream per priority seen, kept for the net's lifetime: switching priorities costs nothing). */
int lrs_dipnet_train_steps(lrs_dipnet *net, const float *x, const float *target, const float *mask,
                           float lr, float beta1, float beta2, float eps, lrs_es_state *es,
                           float *ring, int nsteps, int use_graph, void *stream);
/* The same with a mask of mask_channels channels: 1 = [P] over the output pixels
 * (lrs_dipnet_train_steps is this case), the net's output C = per element [C][H][W], for a mask that
 * differs between bands: loss = MSELoss(target*mask, out*mask) of …1-LiP.py:234 with mask_bkg
 * generalised from (1,1,H,W) to (1,C,H,W).  Any other count returns LRS_E_INVALID before anything is
 * launched.  A captured graph is keyed by the mask mode as well as by the pointers. */
int lrs_dipnet_train_steps_cmask(lrs_dipnet *net, const float *x, const float *target, const float *mask,
                                 int mask_channels, float lr, float beta1, float beta2, float eps,
                                 lrs_es_state *es, float *ring, int nsteps, int use_graph, void *stream);
/* loss of the last step (synchronises the stream; diagnostics only) */
int lrs_dipnet_last_loss(lrs_dipnet *net, double *loss, void *stream);
/* Stream ordering between two streams of one device: work enqueued on `waiter` after this call runs
 * after the work enqueued on `signaler` before it (an event with a device-scope release: cheaper
 * than a default event when nothing on the host waits on it).  The Python side orders the DIP
 * stream against the caller's this way. */
int lrs_stream_wait(void *waiter, void *signaler);

/* ---- Metrics (not timed) -------------------------------------------------------------------
 * acc (device double) = sum of the SSIM map of pytorch_ssim.ssim(img1, img2) over C x H x W
 * (pytorch_ssim/__init__.py:17-37; called at main_LRS_PnP_DIP_1-LiP.py:480-481); MSSIM =
 * acc / (C*H*W).  Images are [C][H][W] float32. */
int lrs_ssim_f32(const float *img1, const float *img2, int C, int H, int W, double *acc, void *stream);
/* Per-band PSNR 10 log10(255 / sqrt(mse_b)) (100 when mse_b < 1e-10) of X against C, both P x B
 * float32 unfolded (main_LRS_PnP.py:379-384, psnr() :40-46, bach_mpsnr :49-58); psnr: device, B
 * doubles.  fp64 accumulation, fixed-order reduction (deterministic). */
size_t lrs_psnr_workspace(int64_t P, int64_t B);
int lrs_psnr_bands_f32(const float *X, const float *C, int64_t P, int64_t B, double *psnr, void *ws,
                       size_t ws_bytes, void *stream);

/* ---- Quality monitor: one pass over X and the clean cube, and a device-side best iterate -------
 * The scores every reference main prints after an outer iteration (main_LRS_PnP.py:368-391: MPSNR against
 * the clean image, best_PSNR), with the region restriction and the spectral angle an inpainting run on a
 * hyperspectral cube is judged by.  X (the solver's X) and C (the clean cube) are [P][B] float32 unfolded;
 * region is NULL (every entry counts) or u8 [P][B], 1 = counted (1 - M scores the hole alone).  All
 * arithmetic is fp64 on the float32 inputs.  With r = region[p][b] (1 when NULL):
 *   n_b = sum_p r,  sse_b = sum_p r (x - c)^2,
 *   psnr_b = 10 log10(255 / sqrt(sse_b / n_b)), 100 when sse_b / n_b < 1e-10 (as lrs_psnr_bands_f32), NaN when
 *            n_b = 0;
 *   q[0] = MPSNR: the mean of psnr_b over the bands with n_b > 0 (NaN when there is none);
 *   q[1] = SAM in degrees: the mean over the counted pixels of acos(clamp(<x_p, c_p> / (|x_p| |c_p|), -1, 1)),
 *          the products over all B bands; a pixel counts when region is NULL or any region[p][.] is 1, and
 *          |x_p| |c_p| > 0 (NaN when none counts);
 *   q[2] = sqrt(sum r (x - c)^2) / sqrt(sum r c^2) (NaN when the denominator is 0);
 *   q[3] = the number of pixels counted for q[1].
 * q: device, 4 doubles.  psnr_bands: NULL or device, B doubles, receives psnr_b.  X, C and region are each
 * read once; every sum has a fixed order (slab partials in ws, no atomics), so reruns and calls on a base
 * misaligned by one float give the same bits.  Any P, B >= 1 with P B < 2^31; B > 512 takes a slower form of
 * the same definition.  Never allocates, never synchronises; every refusal is decided before a launch:
 * LRS_E_INVALID: X, C, q or ws NULL, a size <= 0.  LRS_E_UNSUPPORTED: P B >= 2^31 (the workspace size is 0
 * there).  LRS_E_WORKSPACE: ws_bytes too small. */
size_t lrs_cube_quality_workspace(int64_t P, int64_t B);
int lrs_cube_quality_f32(const float *X, const float *C, const uint8_t *region, int64_t P, int64_t B, double *q,
                         double *psnr_bands, void *ws, size_t ws_bytes, void *stream);
/* Keep the iterate when its score is better, decided on the device (no host read).  score: device, 1 double;
 * best: device, {score, iteration}, initialised by the caller to NaN.  Better: sign * score[0] > sign *
 * best[0], strictly (sign +1: larger is better, -1: smaller); a NaN score never is; a NaN best[0] is beaten
 * by any score that is not NaN.  When better, dst <- src (n floats) and best <- {score[0], iteration};
 * otherwise nothing is written.  Two stream-ordered launches: the copy, in which every workgroup reads best
 * for the decision, then the update of best.  LRS_E_INVALID: a NULL pointer, n <= 0, sign not +1 or -1, src
 * overlapping dst. */
int lrs_keep_best_f32(const double *score, int sign, int32_t iteration, const float *src, float *dst, int64_t n,
                      double *best, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LRSPNP_H */

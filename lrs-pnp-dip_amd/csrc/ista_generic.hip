// The generic sparse-coding path (any K; the only one for K > 512): every inner iteration as two
// dense GEMMs over chunks of blocks, and the stand-alone NLM column kernel that is its prox and the
// denoise_nl_means drop-in (lrs_nlm_col_f32, lrs_nlm_matlab_col_f32).
//
// Reference path (shuoli0708/LRS-PnP-DIP): the per-block loop of main_LRS_PnP.py:270-303 calling
// ista() (:131-149), for all blocks of a chunk at once.
#include <algorithm>

#include "ista_paths.h"
#include "lrs_nlm.h"

namespace lrs {

// Standalone NLM over nvec columns of length K (any K >= 1): one workgroup per column, the
// column reflect-padded in LDS, one thread per output.
__global__ __launch_bounds__(256) void k_nlm_col(const float *__restrict__ g, int64_t ldg,
                                                 float *__restrict__ out, int64_t ldo, int K,
                                                 double h, const double *__restrict__ hv) {
    extern __shared__ float col[];  // K + 10
    const int64_t v = blockIdx.x;
    const float *gv = g + v * ldg;
    const int n = K + 10;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        int s = i - 5;
        if (K > 1) {
            const int period = 2 * (K - 1);
            s %= period;
            if (s < 0) s += period;
            if (s >= K) s = period - s;
        } else {
            s = 0;
        }
        col[i] = gv[s];
    }
    __syncthreads();
    const double hh = hv ? hv[v] : h;
    const double kneg = nlm_kneg(hh);
    const double c0 = nlm_c0();
    for (int i = threadIdx.x; i < K; i += blockDim.x) {
        double w[11];
#pragma unroll
        for (int k = 0; k < 11; ++k) w[k] = (double)col[i + 5 - 3 + k];
        out[v * ldo + i] = nlm_point<3>(w, kneg, c0);
    }
}

// k_nlm_col over nvec columns.  Its dynamic LDS is (K + 10) floats: above 64 KiB (K > 16374) the
// launch must be opted into more (gfx950: 160 KiB per workgroup), once per device.
static int nlm_col_launch(const float *g, int64_t ldg, float *out, int64_t ldo, int64_t K, int64_t nvec, double h,
                          const double *h_per_vec, hipStream_t st) {
    const size_t bytes = (size_t)(K + 10) * sizeof(float);
    static std::atomic<uint64_t> opted{0};
    if (bytes > 65536)
        if (const int rc = lds_opt_in((const void *)k_nlm_col, 160 * 1024, opted)) return rc;
    hipLaunchKernelGGL(k_nlm_col, dim3((unsigned)nvec), dim3(256), bytes, st, g, ldg, out, ldo, (int)K, h, h_per_vec);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// Per chunk of up to kGenChunk blocks, every inner iteration is
//   R = X D^T            (chunk x n, dense GEMM)       r = obs .* (Yb - R)
//   G = r D              (chunk x K, dense GEMM)       g = X + G / alpha        X = prox(g)
// and finally Phi = X D^T.  The products are fp32-accurate (split-bf16 or f32 MFMA), the prox is
// the same kernel as lrs_nlm_col_f32 / lrs_nlm_matlab_col_f32.
constexpr int64_t kGenChunk = 4096;

__global__ void k_gen_resid(float *__restrict__ R, const float *__restrict__ Yb, const uint8_t *__restrict__ obs,
                            int64_t rows, int n, int n_pad) {
    const int64_t total = rows * n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = i / n;
        const int r = (int)(i - j * n);
        R[i] = obs[j * n_pad + r] ? Yb[j * n_pad + r] - R[i] : 0.0f;
    }
}

// g = x + G / alpha (in place in G); the quotient as the oracle / reference ((H^T r) / alpha)
__global__ void k_gen_grad(float *__restrict__ G, const float *__restrict__ X, const float *__restrict__ alpha,
                           int64_t rows, int K) {
    const int64_t total = rows * K;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = i / K;
        G[i] = X[i] + G[i] / alpha[j];
    }
}

__global__ void k_gen_soft(const float *__restrict__ G, float *__restrict__ X, const double *__restrict__ thr,
                           int64_t rows, int K) {
    const int64_t total = rows * K;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const float T = (float)thr[i / K], gv = G[i];
        float t = fabsf(gv) - T;
        t = t > 0.f ? t : 0.f;
        X[i] = gv > 0.f ? t : (gv < 0.f ? -t : 0.f);
    }
}

// FISTA momentum (lrs_ista_opts.accel): X holds x_k after the prox; X <- z_{k+1} = x_k + beta (x_k - x_{k-1}),
// Xprev <- x_k.  beta = 0 (the first iteration) leaves X as it is.
__global__ void k_gen_momentum(float *__restrict__ X, float *__restrict__ Xprev, float beta, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const float xn = X[i];
        if (beta != 0.f) X[i] = xn + beta * (xn - Xprev[i]);
        Xprev[i] = xn;
    }
}

__global__ void k_gen_phi(const float *__restrict__ R, float *__restrict__ phi, int64_t rows, int n, int n_pad) {
    const int64_t total = rows * n_pad;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = i / n_pad;
        const int r = (int)(i - j * n_pad);
        phi[i] = r < n ? R[j * n + r] : 0.0f;
    }
}

static unsigned gen_blocks(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 8192); }

// split-K scratch for any chunk of <= kGenChunk blocks: the split count grows as the tile count falls,
// so the need peaks at the top of each 64-row band, not at the full chunk
static int64_t ista_generic_part_floats(int64_t n, int64_t K) {
    int64_t m = 0;
    for (int64_t rows = 64; rows <= kGenChunk; rows += 64)
        m = std::max(m, std::max(dense_gemm_part_floats((int)rows, (int)n, (int)K),
                                 dense_gemm_part_floats((int)rows, (int)K, (int)n)));
    return m;
}

size_t ista_generic_workspace(int64_t n, int64_t K, bool accel) {
    const int64_t c = kGenChunk;
    return (size_t)((accel ? 3 : 2) * c * K + c * n + ista_generic_part_floats(n, K)) * sizeof(float) + 256;
}

int ista_generic(const float *Yb, const uint8_t *obs, const float *D, int64_t n, int64_t n_pad, int64_t K, int64_t nb,
                 const float *alpha, const double *thr, int Nit, int prox, float *coefs, float *phi, void *ws,
                 size_t ws_bytes, hipStream_t st, bool accel) {
    if (!ws || ws_bytes < ista_generic_workspace(n, K, accel)) return LRS_E_WORKSPACE;
    if (n > INT32_MAX / 2 || K > 16384) return LRS_E_UNSUPPORTED;
    const int64_t c = kGenChunk;
    float *X = (float *)ws, *G = X + c * K, *R = G + c * K, *part = R + c * n;
    const int64_t part_cap = ista_generic_part_floats(n, K);
    float *Xprev = part + part_cap;   // x_{k-1} (accel only: the workspace is that much longer)
    for (int64_t j0 = 0; j0 < nb; j0 += c) {
        const int rows = (int)std::min(c, nb - j0);
        hipError_t e = hipMemsetAsync(X, 0, sizeof(float) * rows * K, st);
        if (e != hipSuccess) return (int)e;
        double tk = 1.0;   // FISTA t_k (fp64, as the fused kernels)
        for (int it = 0; it < Nit; ++it) {
            int rc = dense_gemm(0, 1, X, D, R, rows, (int)n, (int)K, part, part_cap, st);   // R = X D^T
            if (rc) return rc;
            hipLaunchKernelGGL(k_gen_resid, dim3(gen_blocks(rows * n)), dim3(256), 0, st, R, Yb + j0 * n_pad,
                               obs + j0 * n_pad, (int64_t)rows, (int)n, (int)n_pad);
            rc = dense_gemm(0, 0, R, D, G, rows, (int)K, (int)n, part, part_cap, st);          // G = r D
            if (rc) return rc;
            hipLaunchKernelGGL(k_gen_grad, dim3(gen_blocks(rows * K)), dim3(256), 0, st, G, X, alpha + j0,
                               (int64_t)rows, (int)K);
            if (prox == LRS_PROX_SOFT) {
                hipLaunchKernelGGL(k_gen_soft, dim3(gen_blocks(rows * K)), dim3(256), 0, st, G, X, thr + j0,
                                   (int64_t)rows, (int)K);
            } else if (prox == LRS_PROX_NLM_MATLAB) {
                rc = nlm_matlab_col_launch(G, K, X, K, K, rows, 0.0, thr + j0, st);
                if (rc) return rc;
            } else {
                rc = nlm_col_launch(G, K, X, K, K, rows, 0.0, thr + j0, st);
                if (rc) return rc;
            }
            if (accel) {
                const double tn = 0.5 * (1.0 + sqrt(1.0 + 4.0 * tk * tk));
                const float beta = (float)((tk - 1.0) / tn);
                tk = tn;
                if (it + 1 < Nit)   // the last iteration leaves x_Nit itself
                    hipLaunchKernelGGL(k_gen_momentum, dim3(gen_blocks(rows * K)), dim3(256), 0, st, X, Xprev, beta,
                                       (int64_t)rows * K);
            }
            LRS_CHECK_LAUNCH();
        }
        int rc = dense_gemm(0, 1, X, D, R, rows, (int)n, (int)K, part, part_cap, st);          // Phi = X D^T
        if (rc) return rc;
        hipLaunchKernelGGL(k_gen_phi, dim3(gen_blocks(rows * n_pad)), dim3(256), 0, st, R, phi + j0 * n_pad,
                           (int64_t)rows, (int)n, (int)n_pad);
        if (coefs) {
            e = hipMemcpyAsync(coefs + j0 * K, X, sizeof(float) * rows * K, hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) return (int)e;
        }
        LRS_CHECK_LAUNCH();
    }
    return LRS_OK;
}

}  // namespace lrs

using namespace lrs;

extern "C" int lrs_nlm_col_f32(const float *g, int64_t ldg, float *out, int64_t ldo, int64_t K,
                               int64_t nvec, double h, const double *h_per_vec, int patch_size,
                               int patch_distance, void *stream) {
    if (!g || !out || K <= 0 || nvec < 0 || ldg < K || ldo < K) return LRS_E_INVALID;
    if (patch_size != 3 || patch_distance != 3) return LRS_E_UNSUPPORTED;
    if (K > 16384) return LRS_E_UNSUPPORTED;
    if (nvec == 0) return LRS_OK;
    return nlm_col_launch(g, ldg, out, ldo, K, nvec, h, h_per_vec, (hipStream_t)stream);
}

extern "C" int lrs_nlm_matlab_col_f32(const float *g, int64_t ldg, float *out, int64_t ldo, int64_t K,
                                      int64_t nvec, double h, const double *h_per_vec, void *stream) {
    if (!g || !out || K <= 0 || nvec < 0 || ldg < K || ldo < K) return LRS_E_INVALID;
    if (K > 16384) return LRS_E_UNSUPPORTED;
    if (nvec == 0) return LRS_OK;
    return nlm_matlab_col_launch(g, ldg, out, ldo, K, nvec, h, h_per_vec, (hipStream_t)stream);
}

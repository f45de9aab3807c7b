// DIP low-rank prox primitives: the layers of the 1-Lipschitz U-Net and its training step.
// This header: what the primitive C ABI and every other DIP header share -- the dense fp32 GEMMs and
// k_gemm_reduce, im2col / col2im, the block sums, the activations, concat.  The rest by stage:
//   dip_bn.h     BatchNorm (+ Lipschitz rescale, + activation), every form, and which form serves a shape
//   dip_sn.h     sigma_max of the conv weights (Gram, Lanczos + Sturm) and W / scale
//   dip_train.h  loss heads, Adam, the step's begin, early stopping
//   dip_gemm.h / dip_pw.h / dip_sm.h / dip_dir.h   the split-bf16, pointwise, small-map and direct conv products
//   dip_wprep.h  the per-step weight planes;  dip_dgrad.h  the kernels that finish a data gradient
//   dip_image.h  image transforms, parameter initialisation
//
// Reference (shuoli0708/LRS-PnP-DIP):
//   models/my_Lipschitz_Unet.py:21-148        the network (conv / bn / act stack)
//   models/lipschitz_constraint_layer.py:6-22   act(): LeakyReLU(0.2, inplace=True)
//   lipschitz_constraint_layer.py:36-44         SpectralNorm._update_u_v: sigma = svd(W.view(Co,-1))[0],
//                                               W = W_bar / max(1, sigma / ln_lambda)
//   lipschitz_constraint_layer.py:65-78         conv(): ReflectionPad2d((k-1)//2) + Conv2d(pad 0)
//   lipschitz_constraint_layer.py:88-101,113-122  BatchNormSpectralNorm: gamma/c, beta/c with
//                                               c = max(max|gamma_orig|, 1) (no grad through c)
//   main_LRS_PnP_DIP_1-LiP.py:214-237           Adam(lr), MSELoss(target*mask, out*mask)
//
// MI355X design: activations are [C][H][W] fp32 (batch 1, as the reference).  A conv is an
// explicit im2col (reflection pad / stride / nearest x2 upsample folded into the gather) and an
// MFMA f32 GEMM; the backward is the same GEMM transposed (dW = dZ col^T with split-K, dcol =
// Wn^T dZ) plus a deterministic col2im gather that also applies the adjoints of the padding and
// the upsample.  BatchNorm (train-mode batch statistics) + LeakyReLU are one kernel per
// direction, one workgroup per channel, statistics in fp64.  sigma_max of every conv weight is
// computed exactly (not by power iteration): fp64 Gram on the smaller side, then Lanczos with
// the Gram held in registers and a 256-way parallel Sturm multisection for the top eigenvalue.
#include <math.h>

#include "lrs_common.h"
#include "lrs_dip.h"

// Kernel definitions; part of dipnet.hip's translation unit (and of the tools/micro programs).
#pragma once

namespace lrs {

// ------------------------------------------------------------------------------------------
// GEMM  C[M][N] = op(A)[M][K] * op(B)[K][N]   (fp32, v_mfma_f32_16x16x4_f32)
//   TA = 0: A stored [M][K];  TA = 1: A stored [K][M]
//   TB = 0: B stored [K][N];  TB = 1: B stored [N][K]
// 128x128 tile per 256-thread workgroup (2x2 waves of 64x64 = 4x4 MFMA tiles), BK = 16.
// Both operands sit in LDS k-contiguous ([x][BK+4] floats), so each lane fetches the four
// k-steps of an MFMA fragment with one ds_read_b128; two LDS stages, one barrier per k-step,
// the next k-step's global loads in flight during the MFMAs.
// gridDim.z > 1 = split-K: partial z goes to Cpart + z*M*N and k_gemm_reduce finishes.
// ------------------------------------------------------------------------------------------
constexpr int kBM = 128, kBN = 128, kBK = 16, kGemmThreads = 256, kLdsK = kBK + 4;

struct GemmArgs {
    const float *A, *B;
    float *C;            // final output (split == 1) or partial base (split > 1)
    const float *bias;   // [M] or null (split == 1 only)
    const float *div;    // scalar divisor (device) or null (split == 1 only)
    int M, N, K, kchunk;
    int accum;           // final C += result instead of C = result
    // k_gemm_s3 only: ncls > 1 output parity classes of an upsampled conv (gridDim.z = ncls x
    // splits; column n of class cls = 2 i + j is source pixel (a, b) = (n / cls_ws, n % cls_ws),
    // stored at output pixel (2a + i) cls_wo + 2b + j of rows of ldc floats)
    int ncls, cls_ws, cls_wo;
    int64_t ldc;         // output row length (0: N)
};

// A 128(x) x 16(k) operand tile, 8 values per thread, as two float4 of 4 consecutive k.
//  KCONTIG: stored [x][k] (k contiguous): thread -> x = t/2, k = 8 (t&1) + 0..7
//  else   : stored [k][x] (x contiguous): thread -> x = t&127, k = 8 (t>>7) + 0..7
template <bool KCONTIG>
__device__ __forceinline__ void load_tile(const float *__restrict__ S, int ld, int k0, int kend, int x0, int X,
                                          float4 (&r)[2]) {
    const int t = threadIdx.x;
    if (KCONTIG) {
        const int x = x0 + (t >> 1), kb = k0 + 8 * (t & 1);
        const float *src = S + (int64_t)x * ld;
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = (x < X && kb + u < kend) ? src[kb + u] : 0.0f;
        r[0] = float4{v[0], v[1], v[2], v[3]};
        r[1] = float4{v[4], v[5], v[6], v[7]};
    } else {
        const int x = x0 + (t & 127), kb = k0 + 8 * (t >> 7);
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = (x < X && kb + u < kend) ? S[(int64_t)(kb + u) * ld + x] : 0.0f;
        r[0] = float4{v[0], v[1], v[2], v[3]};
        r[1] = float4{v[4], v[5], v[6], v[7]};
    }
}

template <bool KCONTIG>
__device__ __forceinline__ void store_tile(float (*T)[kLdsK], const float4 (&r)[2]) {
    const int t = threadIdx.x;
    const int x = KCONTIG ? (t >> 1) : (t & 127);
    const int kb = KCONTIG ? 8 * (t & 1) : 8 * (t >> 7);
    *reinterpret_cast<float4 *>(&T[x][kb]) = r[0];
    *reinterpret_cast<float4 *>(&T[x][kb + 4]) = r[1];
}

template <int TA, int TB>
__global__ __launch_bounds__(kGemmThreads) void k_gemm(GemmArgs g) {
    __shared__ __attribute__((aligned(16))) float As[2][kBM][kLdsK];
    __shared__ __attribute__((aligned(16))) float Bs[2][kBN][kLdsK];
    const int m0 = blockIdx.y * kBM, n0 = blockIdx.x * kBN;
    const int kbeg = blockIdx.z * g.kchunk;
    const int kend = min(g.K, kbeg + g.kchunk);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wm = (wv >> 1) * 64, wn = (wv & 1) * 64;
    const int jl = lane & 15, gk = lane >> 4;
    const int lda = TA ? g.M : g.K;
    const int ldb = TB ? g.K : g.N;
    floatx4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = floatx4{0.f, 0.f, 0.f, 0.f};
    float4 ra[2], rb[2];
    load_tile<TA == 0>(g.A, lda, kbeg, kend, m0, g.M, ra);
    load_tile<TB == 1>(g.B, ldb, kbeg, kend, n0, g.N, rb);
    int stage = 0;
    store_tile<TA == 0>(As[0], ra);
    store_tile<TB == 1>(Bs[0], rb);
    __syncthreads();
    for (int k0 = kbeg; k0 < kend; k0 += kBK) {
        const bool more = k0 + kBK < kend;
        if (more) {
            load_tile<TA == 0>(g.A, lda, k0 + kBK, kend, m0, g.M, ra);
            load_tile<TB == 1>(g.B, ldb, k0 + kBK, kend, n0, g.N, rb);
        }
        float4 fa[4], fb[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) fa[a] = *reinterpret_cast<const float4 *>(&As[stage][wm + 16 * a + jl][4 * gk]);
#pragma unroll
        for (int b = 0; b < 4; ++b) fb[b] = *reinterpret_cast<const float4 *>(&Bs[stage][wn + 16 * b + jl][4 * gk]);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                acc[a][b] = mfma16x16x4(fa[a].x, fb[b].x, acc[a][b]);
                acc[a][b] = mfma16x16x4(fa[a].y, fb[b].y, acc[a][b]);
                acc[a][b] = mfma16x16x4(fa[a].z, fb[b].z, acc[a][b]);
                acc[a][b] = mfma16x16x4(fa[a].w, fb[b].w, acc[a][b]);
            }
        if (more) {
            store_tile<TA == 0>(As[stage ^ 1], ra);   // the other stage: last read one step ago
            store_tile<TB == 1>(Bs[stage ^ 1], rb);
        }
        __syncthreads();
        stage ^= 1;
    }
    float *C = g.C + (int64_t)blockIdx.z * g.M * g.N;
    const bool final_out = gridDim.z == 1;
    const float dv = (final_out && g.div) ? *g.div : 1.0f;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int n = n0 + wn + 16 * b + jl;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + 16 * a + 4 * gk + r;
                if (m < g.M && n < g.N) {
                    float v = acc[a][b][r];
                    if (final_out) {
                        if (g.bias) v = v + g.bias[m];
                        if (g.div) v = v / dv;
                        if (g.accum) v = C[(int64_t)m * g.N + n] + v;
                    }
                    C[(int64_t)m * g.N + n] = v;
                }
            }
        }
}

// k-step of the split-bf16 128x128 GEMM (k_gemm_s3, dip_gemm.h): choose_split rounds its k-chunks to it
constexpr int kBK32 = 32;

// ---- small-tile variant (64x64, BK 16, 2x2 waves of 32x32) for GEMMs whose 128-tile grid is
// too small to fill the chip (the 36x36 native U-Net layers) ----------------------------------
constexpr int kBM64 = 64, kBN64 = 64, kBK64 = 16;

// Load a 16(k) x 64(x) operand tile into 4 registers per thread.
//  kmajor = stored [k][x] (contiguous along x), else stored [x][k] (contiguous along k).
template <bool KMAJOR>
__device__ __forceinline__ void load_tile64(const float *__restrict__ S, int ld, int k0, int kend, int x0, int X,
                                          float (&r)[4]) {
    const int t = threadIdx.x;
    if (KMAJOR) {
        const int kk = t >> 4, i = (t & 15) * 4;
        const int k = k0 + kk;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int x = x0 + i + u;
            r[u] = (k < kend && x < X) ? S[(int64_t)k * ld + x] : 0.0f;
        }
    } else {
        const int i = t >> 2, kk = (t & 3) * 4;
        const int x = x0 + i;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + kk + u;
            r[u] = (k < kend && x < X) ? S[(int64_t)x * ld + k] : 0.0f;
        }
    }
}

template <bool KMAJOR>
__device__ __forceinline__ void store_tile64(float (*T)[kBM64 + 4], const float (&r)[4]) {
    const int t = threadIdx.x;
    if (KMAJOR) {
        const int kk = t >> 4, i = (t & 15) * 4;
#pragma unroll
        for (int u = 0; u < 4; ++u) T[kk][i + u] = r[u];
    } else {
        const int i = t >> 2, kk = (t & 3) * 4;
#pragma unroll
        for (int u = 0; u < 4; ++u) T[kk + u][i] = r[u];
    }
}

template <int TA, int TB>
__global__ __launch_bounds__(kGemmThreads) void k_gemm64(GemmArgs g) {
    __shared__ float As[kBK64][kBM64 + 4];
    __shared__ float Bs[kBK64][kBN64 + 4];
    const int m0 = blockIdx.y * kBM64, n0 = blockIdx.x * kBN64;
    const int kbeg = blockIdx.z * g.kchunk;
    const int kend = min(g.K, kbeg + g.kchunk);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wm = (wv >> 1) * 32, wn = (wv & 1) * 32;
    const int jl = lane & 15, gk = lane >> 4;
    // A: TA=0 stored [M][K] -> contiguous along k (x-major); TA=1 stored [K][M] (k-major)
    const int lda = TA ? g.M : g.K;
    const int ldb = TB ? g.K : g.N;
    floatx4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = floatx4{0.f, 0.f, 0.f, 0.f};
    float ra[4], rb[4];
    load_tile64<TA == 1>(g.A, lda, kbeg, kend, m0, g.M, ra);
    load_tile64<TB == 0>(g.B, ldb, kbeg, kend, n0, g.N, rb);
    for (int k0 = kbeg; k0 < kend; k0 += kBK64) {
        store_tile64<TA == 1>(As, ra);
        store_tile64<TB == 0>(Bs, rb);
        __syncthreads();
        if (k0 + kBK64 < kend) {
            load_tile64<TA == 1>(g.A, lda, k0 + kBK64, kend, m0, g.M, ra);
            load_tile64<TB == 0>(g.B, ldb, k0 + kBK64, kend, n0, g.N, rb);
        }
#pragma unroll
        for (int s = 0; s < kBK64 / 4; ++s) {
            const float a0 = As[4 * s + gk][wm + jl], a1 = As[4 * s + gk][wm + 16 + jl];
            const float b0 = Bs[4 * s + gk][wn + jl], b1 = Bs[4 * s + gk][wn + 16 + jl];
            acc[0][0] = mfma16x16x4(a0, b0, acc[0][0]);
            acc[0][1] = mfma16x16x4(a0, b1, acc[0][1]);
            acc[1][0] = mfma16x16x4(a1, b0, acc[1][0]);
            acc[1][1] = mfma16x16x4(a1, b1, acc[1][1]);
        }
        __syncthreads();
    }
    float *C = g.C + (int64_t)blockIdx.z * g.M * g.N;
    const bool final_out = gridDim.z == 1;
    const float dv = (final_out && g.div) ? *g.div : 1.0f;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int n = n0 + wn + 16 * b + jl;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + 16 * a + 4 * gk + r;
                if (m < g.M && n < g.N) {
                    float v = acc[a][b][r];
                    if (final_out) {
                        if (g.bias) v = v + g.bias[m];
                        if (g.div) v = v / dv;
                        if (g.accum) v = C[(int64_t)m * g.N + n] + v;
                    }
                    C[(int64_t)m * g.N + n] = v;
                }
            }
        }
}

// C = (sum_z part[z]) (+ bias[m]) (/ *div): fixed summation order (deterministic); 8 partial
// chains so the loads of a long split stay in flight
__global__ void k_gemm_reduce(const float *__restrict__ part, int nsplit, int M, int N, const float *bias,
                              const float *div, int accum, float *__restrict__ C) {
    const int64_t MN = (int64_t)M * N;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= MN) return;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int z = 0;
    for (; z + 8 <= nsplit; z += 8)
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] += part[(int64_t)(z + u) * MN + i];
    for (; z < nsplit; ++z) acc[z & 7] += part[(int64_t)z * MN + i];
    float s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    if (bias) s = s + bias[i / N];
    if (div) s = s / *div;
    if (accum) s = C[i] + s;
    C[i] = s;
}

// ------------------------------------------------------------------------------------------
// im2col / col2im with nearest x2 upsample and reflection / zero padding folded in.
//   source x: [C][Hs][Ws];  upsampled (Hu, Wu) = up ? (2Hs, 2Ws) : (Hs, Ws);
//   padded coordinate iy in [0, Hu + 2 pad);  col[(c*k + ky)*k + kx][oy*Wo + ox] =
//   xsrc(c, iy = oy*stride + ky, ix = ox*stride + kx)   (torch weight order [co][ci][ky][kx])
// ------------------------------------------------------------------------------------------
// ReflectionPad2d (no edge repeat) folded once: for -n < u < 2n - 1, which pad < n guarantees.
// (ista_prox.h's reflect_idx is the periodic numpy 'reflect' for any overhang: another function.)
__device__ __forceinline__ int reflect_once_idx(int u, int n) {
    if (u < 0) u = -u;
    if (u >= n) u = 2 * (n - 1) - u;
    return u;
}

// One col row r = (c, ky, kx) per blockIdx.y (grid-strided), the output pixels of that row across
// blockIdx.x: 32-bit index arithmetic, c / ky / kx uniform per workgroup.
__global__ __launch_bounds__(256) void k_im2col(const float *__restrict__ x, ConvGeom gm, float *__restrict__ col) {
    const int P = gm.Ho * gm.Wo, kk = gm.k * gm.k, Kc = gm.Cin * kk;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int oy = p / gm.Wo, ox = p - oy * gm.Wo;
    for (int r = blockIdx.y; r < Kc; r += gridDim.y) {
        const int c = r / kk, kyx = r - c * kk, ky = kyx / gm.k, kx = kyx - ky * gm.k;
        int uy = oy * gm.stride + ky - gm.pad, ux = ox * gm.stride + kx - gm.pad;
        float v = 0.0f;
        bool inside = true;
        if (gm.pad_mode == LRS_PAD_REFLECT) {
            uy = reflect_once_idx(uy, gm.Hu);
            ux = reflect_once_idx(ux, gm.Wu);
        } else {
            inside = uy >= 0 && uy < gm.Hu && ux >= 0 && ux < gm.Wu;
        }
        if (inside) {
            const int sy = gm.up ? (uy >> 1) : uy, sx = gm.up ? (ux >> 1) : ux;
            v = x[((int64_t)c * gm.Hs + sy) * gm.Ws + sx];
        }
        col[(int64_t)r * P + p] = v;
    }
}

// Padded positions that read upsampled index u (n = upsampled extent): the direct one and, for
// reflection, the top/left mirror (u in [1, pad]) and the bottom/right mirror
// (u in [n-1-pad, n-2]); a tiny extent can have all three.
// kPadClamp (internal, pad 1 only): the border index also takes the position just outside it --
// the source-grid form of an upsampled reflection-padded conv (k_gemm_s3's parity classes)
constexpr int kPadClamp = 2;
__device__ __forceinline__ int padded_sources(int u, int n, int pad, int mode, int (&iy)[3]) {
    int cnt = 0;
    iy[cnt++] = u + pad;
    if (mode == LRS_PAD_REFLECT && pad > 0) {
        if (u >= 1 && u <= pad) iy[cnt++] = pad - u;
        if (u >= n - 1 - pad && u <= n - 2) iy[cnt++] = 2 * (n - 1) - u + pad;
    } else if (mode == kPadClamp) {
        if (u == 0) iy[cnt++] = 0;
        if (u == n - 1) iy[cnt++] = n + 1;
    }
    return cnt;
}

// dx[c][y][x] = sum over every col entry that read it (adjoint of k_im2col), gather form.  One
// channel per blockIdx.y (grid-strided), its pixels across blockIdx.x; 32-bit index arithmetic and
// the stride as a template parameter (1 and 2 are the nets' strides).
template <int STRIDE>
__device__ __forceinline__ float col2im_pixel(const float *__restrict__ dcol, const ConvGeom &gm, int c, int sy,
                                              int sx, int P) {
    const int k = gm.k;
    const int s = STRIDE > 0 ? STRIDE : gm.stride;
    float acc = 0.0f;
    const int nup = gm.up ? 2 : 1;
    for (int a = 0; a < nup; ++a) {
        const int uy = gm.up ? 2 * sy + a : sy;
        int iys[3];
        const int ny = padded_sources(uy, gm.Hu, gm.pad, gm.pad_mode, iys);
        for (int b = 0; b < nup; ++b) {
            const int ux = gm.up ? 2 * sx + b : sx;
            int ixs[3];
            const int nx = padded_sources(ux, gm.Wu, gm.pad, gm.pad_mode, ixs);
            for (int py = 0; py < ny; ++py)
                for (int ky = 0; ky < k; ++ky) {
                    const int ty = iys[py] - ky;
                    if (ty < 0 || ty % s) continue;
                    const int oy = ty / s;
                    if (oy >= gm.Ho) continue;
                    for (int px = 0; px < nx; ++px)
                        for (int kx = 0; kx < k; ++kx) {
                            const int tx = ixs[px] - kx;
                            if (tx < 0 || tx % s) continue;
                            const int ox = tx / s;
                            if (ox >= gm.Wo) continue;
                            acc += dcol[(int64_t)((c * k + ky) * k + kx) * P + oy * gm.Wo + ox];
                        }
                }
        }
    }
    return acc;
}

template <int STRIDE>
__global__ __launch_bounds__(256) void k_col2im(const float *__restrict__ dcol, ConvGeom gm, float *__restrict__ dx,
                                                int accum) {
    const int HW = gm.Hs * gm.Ws, P = gm.Ho * gm.Wo;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= HW) return;
    const int sy = q / gm.Ws, sx = q - sy * gm.Ws;
    for (int c = blockIdx.y; c < gm.Cin; c += gridDim.y) {
        const float acc = col2im_pixel<STRIDE>(dcol, gm, c, sy, sx, P);
        const int64_t i = (int64_t)c * HW + q;
        dx[i] = accum ? dx[i] + acc : acc;
    }
}

// ------------------------------------------------------------------------------------------
// Block reductions over wave_sum_butterfly (lrs_common.h: DPP row operations, no LDS crossbar).
// ------------------------------------------------------------------------------------------
// block sum; red must hold 2 * (blockDim/64) doubles; `parity` alternates between calls so a
// single barrier suffices (the other half of red is still being read by slow waves)
__device__ __forceinline__ double block_sum_d1(double v, double *red, int &parity) {
    const int nw = blockDim.x >> 6;
    v = wave_sum_butterfly(v);
    double *r = red + parity * nw;
    if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < nw; ++i) s += r[i];
    parity ^= 1;
    return s;
}

__device__ __forceinline__ double block_sum_d(double v, double *red) {
    int parity = 0;
    const double s = block_sum_d1(v, red, parity);
    __syncthreads();
    return s;
}

// Two / three block sums behind ONE barrier (red >= 2 / 3 x blockDim / 64 doubles): each sum is
// formed exactly as block_sum_d1 forms it (wave sums, then the waves' values in wave order from
// 0.0), so the results are bitwise those of consecutive block_sum_d1 calls; every thread gets them.
__device__ __forceinline__ void block_sum2_d(double &a, double &b, double *red) {
    const int nw = blockDim.x >> 6, w = threadIdx.x >> 6;
    a = wave_sum_butterfly(a);
    b = wave_sum_butterfly(b);
    if ((threadIdx.x & 63) == 0) {
        red[w] = a;
        red[nw + w] = b;
    }
    __syncthreads();
    double s0 = 0.0, s1 = 0.0;
    for (int i = 0; i < nw; ++i) {
        s0 += red[i];
        s1 += red[nw + i];
    }
    a = s0;
    b = s1;
}

__device__ __forceinline__ void block_sum3_d(double &a, double &b, double &c, double *red) {
    const int nw = blockDim.x >> 6, w = threadIdx.x >> 6;
    a = wave_sum_butterfly(a);
    b = wave_sum_butterfly(b);
    c = wave_sum_butterfly(c);
    if ((threadIdx.x & 63) == 0) {
        red[w] = a;
        red[nw + w] = b;
        red[2 * nw + w] = c;
    }
    __syncthreads();
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < nw; ++i) {
        s0 += red[i];
        s1 += red[nw + i];
        s2 += red[2 * nw + i];
    }
    a = s0;
    b = s1;
    c = s2;
}

// activations (BatchNorm's kernels, dip_bn.h; the k_pw epilogue and the loss heads)
__device__ __forceinline__ float act_fwd(float v, int act) {
    if (act == LRS_ACT_LRELU) return v > 0.0f ? v : v * 0.2f;
    if (act == LRS_ACT_SIGMOID) return 1.0f / (1.0f + expf(-v));
    return v;
}

__device__ __forceinline__ float act_bwd(float g, float y, int act) {
    if (act == LRS_ACT_LRELU) return y > 0.0f ? g : g * 0.2f;
    if (act == LRS_ACT_SIGMOID) return g * (1.0f - y) * y;
    return g;
}

// ------------------------------------------------------------------------------------------
// Concat (models/common.py:11-42): out = cat(a, up2?(b)) along channels, both centre-cropped to
// the smaller H and W (offset (size - target) // 2, :27-37).
// ------------------------------------------------------------------------------------------
struct CatGeom {
    int Ca, Ha, Wa, Cb, Hb, Wb, upb;   // b is (Cb, Hb, Wb) before the optional nearest x2
    int H, W;                          // output spatial size
    int oay, oax, oby, obx;            // crop offsets into a and into up2(b)
};

// Forward: grid (row quads, channels), a thread = 4 consecutive x of one row of one channel; no 64-bit
// division per element, float4 stores when the rows are multiples of 4.
__global__ __launch_bounds__(256) void k_concat_fwd4(const float *__restrict__ a, const float *__restrict__ b,
                                                     CatGeom g, float *__restrict__ out) {
    const int W4 = (g.W + 3) >> 2;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= g.H * W4) return;
    const int c = blockIdx.y, y = t / W4, x0 = 4 * (t - y * W4);
    float v[4];
    if (c < g.Ca) {
        const float *src = a + ((int64_t)c * g.Ha + y + g.oay) * g.Wa + g.oax;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = x0 + e < g.W ? src[x0 + e] : 0.0f;
    } else {
        int yy = y + g.oby;
        if (g.upb) yy >>= 1;
        const float *src = b + ((int64_t)(c - g.Ca) * g.Hb + yy) * g.Wb;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int xx = x0 + e + g.obx;
            if (g.upb) xx >>= 1;
            v[e] = x0 + e < g.W ? src[xx] : 0.0f;
        }
    }
    float *dst = out + ((int64_t)c * g.H + y) * g.W + x0;
    if ((g.W & 3) == 0) {
        *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (x0 + e < g.W) dst[e] = v[e];
    }
}

// Backward: the output gradient gathered back (zeros outside the crop; the 2x2 children of an
// upsampled b pixel are summed, dy then dx); acc: accumulate onto gx.
// part 0: ga over (Ha rows x Wa), channels Ca; part 1: gb over (Hb x Wb), channels Cb
__global__ __launch_bounds__(256) void k_concat_bwd4(const float *__restrict__ go, CatGeom g, float *__restrict__ gx,
                                                     int acc, int part) {
    const int Hs = part ? g.Hb : g.Ha, Ws = part ? g.Wb : g.Wa;
    const int W4 = (Ws + 3) >> 2;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= Hs * W4) return;
    const int c = blockIdx.y, Y = t / W4, X0 = 4 * (t - Y * W4);
    const int64_t HW = (int64_t)g.H * g.W;
    float v[4];
    if (part == 0) {
        const float *gc = go + (int64_t)c * HW;
        const int y = Y - g.oay;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int x = X0 + e - g.oax;
            v[e] = (y >= 0 && y < g.H && x >= 0 && x < g.W && X0 + e < Ws) ? gc[(int64_t)y * g.W + x] : 0.0f;
        }
    } else {
        const float *gc = go + (int64_t)(g.Ca + c) * HW;
        const int f = g.upb ? 2 : 1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float s = 0.0f;
            for (int dy = 0; dy < f; ++dy)
                for (int dx = 0; dx < f; ++dx) {
                    const int y = Y * f + dy - g.oby, x = (X0 + e) * f + dx - g.obx;
                    if (y >= 0 && y < g.H && x >= 0 && x < g.W) s += gc[(int64_t)y * g.W + x];
                }
            v[e] = s;
        }
    }
    float *dst = gx + ((int64_t)c * Hs + Y) * Ws + X0;
    if ((Ws & 3) == 0) {
        float4 r = make_float4(v[0], v[1], v[2], v[3]);
        if (acc) {
            const float4 o = *reinterpret_cast<const float4 *>(dst);
            r = make_float4(o.x + r.x, o.y + r.y, o.z + r.z, o.w + r.w);
        }
        *reinterpret_cast<float4 *>(dst) = r;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (X0 + e < Ws) dst[e] = acc ? dst[e] + v[e] : v[e];
    }
}

}  // namespace lrs

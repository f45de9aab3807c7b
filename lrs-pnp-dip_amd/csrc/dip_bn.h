// DIP low-rank prox, BatchNorm2d (train mode, batch 1) with the Lipschitz rescale, + activation: every
// form of it, and the one place that picks the form for a shape.
//
// Reference: lipschitz_constraint_layer.py:88-101,113-122 (BatchNormSpectralNorm: gamma / c, beta / c with
// c = max(max|gamma_orig|, 1), no gradient through c) and torch's BatchNorm2d.
//
// BatchNorm's arithmetic is edited here only.  Shared by every kernel below and k_conv_bn_dir (dip_dir.h):
//   bn_fwd_stat, bn_fwd_store        mean, clamped variance, invstd; their stores and the running statistics
//                                    (bn_fwd_finish = both, for the one-workgroup forms)
//   splitk_value1 / splitk_value4    a value of z from a product's split-K partials (/ scale, + bias)
//   bn_norm_act                      normalise + affine + activation (scalar and float4): all five sites
//   bn_act_bwd, bn_needs_y           g = act'(dL/dy) from the pre-activation or from y
//   bn_bwd_out                       dL/dz = k (g - mean(g) - x_hat mean(g x_hat)): the backward's four sites
// Still spelled per kernel, because a shared helper changed those kernels' register allocation (DESIGN.md,
// "One header for the DIP BatchNorm family"): k_conv_bn_dir's forward statistics (bn_fwd_stat's
// arithmetic on running statistics it fetched early), the backward's element step in its six loops and
// its finish (mean(g), mean(g x_hat), gradients) at its three sites.
// The forms:
//   k_bn_stats + k_bn_apply, k_bn_bwd_stats + k_bn_bwd_apply   each channel split over S workgroups
//   k_bn_fwd1, k_bn_bwd1                                       one workgroup per channel (P <= 4096)
//   k_reduce_bn1, k_reduce_bn_bwd1                             ... that also finishes a split-K sum
//   k_bn_fwd_r<NQ>, k_bn_bwd_r<NQ>                             the channel held in registers (P <= 40960)
// Host part (the end of the file): bn_split, bn_one_wg, bn_reg_q, bn1_threads pick the form and the
// launch_* helpers own the template dispatch; bn_fwd / bn_bwd (dip_launch.h), plan_bn_fwd / plan_grads
// (dipnet_plan.h) and the engine (dipnet.hip) read the form from them.
#pragma once
#include <math.h>

#include "lrs_common.h"
#include "lrs_dip.h"
#include "dip_kernels.h"   // block_sum2_d / block_sum3_d, act_fwd / act_bwd

namespace lrs {

// Each channel is split over S workgroups (grid = S x C), statistics as per-workgroup fp64 partials
// summed in a fixed order by the apply kernel's thread 0; or one workgroup owns the channel.
constexpr int kBnThreads = 256;
constexpr int kBn1Threads = 1024;   // one workgroup per channel (S == 1): 16 waves share the channel
// ... and on small maps (P <= 4 * kBn1Small: the 25^2 and smaller maps at 196^2, 18^2 and smaller at
// 36^2), where 1024 threads would leave most lanes idle, 256 threads (bn1_threads, below)
constexpr int kBn1Small = 256;

// element i of a [C][P] tensor summed over nsplit split-K partials (stride MN): acc[e] = the splits
// e, e + 8, ... in increasing order (k_gemm_reduce's order), the loads of one group of 8 predicated.
// (Every load of up to 32 splits issued before the first add measured slower: 36^2 step 0.635 ->
// 0.671 ms, 196^2 1.244 -> 1.272, tuning build, 2 interleaved rounds.)
__device__ __forceinline__ float splitk_sum1(const float *__restrict__ part, int nsplit, int64_t MN, int64_t i) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int z0 = 0; z0 < nsplit; z0 += 8) {
        float p[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) p[e] = z0 + e < nsplit ? part[(int64_t)(z0 + e) * MN + i] : 0.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (z0 + e < nsplit) acc[e] += p[e];
    }
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
}

// A value of z of channel c from a product's split-K partials: the partials summed in k_gemm_reduce's
// order (splitk_sum1 / splitk_sum4), / *sdiv if given, + bias[c] if given.  sdiv: the conv ran on the raw
// weights W_bar (the spectral-norm scale not yet known when it was launched, dipnet_step's overlapped
// sigma): z = sum / scale + bias, the same order as the scaled path's epilogue (W / scale) x + bias up to
// the rounding of the quotient's place.
__device__ __forceinline__ float splitk_value1(const float *part, int nsplit, int64_t MN, int64_t i, const float *sdiv,
                                               const float *bias, int c) {
    float v = splitk_sum1(part, nsplit, MN, i);
    if (sdiv) v = v / *sdiv;
    if (bias) v = v + bias[c];
    return v;
}

// c = max(max|gamma_orig|, 1.0) (lipschitz_constraint_layer.py:93-97); whole block, C <= 4 * blockDim
__device__ float bn_lip_scale(const float *gamma, int C, float *redf) {
    float m = 0.0f;
    for (int i = threadIdx.x; i < C; i += blockDim.x) m = fmaxf(m, fabsf(gamma[i]));
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) redf[threadIdx.x >> 6] = m;
    __syncthreads();
    float r = 0.0f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) r = fmaxf(r, redf[i]);
    return fmaxf(r, 1.0f);
}

// The same scale computed by every wave on its own (no barrier): the maximum of the same set of
// |gamma|, so bitwise bn_lip_scale's value
__device__ __forceinline__ float bn_lip_scale_w(const float *gamma, int C) {
    float m = 0.0f;
    for (int i = threadIdx.x & 63; i < C; i += 64) m = fmaxf(m, fabsf(gamma[i]));
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    return fmaxf(m, 1.0f);
}


struct BnArgs {
    const float *z;              // [C][P] conv output
    float *y;                    // [C][P] activation output (may alias z when !bn)
    const float *gamma, *beta;   // bn params (orig), null when !bn
    float *mean, *invstd;        // [C] saved statistics
    float *run_mean, *run_var;   // [C] running statistics (momentum update), nullable
    double *part;                // [C][S][3] partials
    int C, P, S, chunk, bn, act;
    float eps, momentum;
    int lip;                     // BatchNormSpectralNorm rescale (1-Lip) or plain BatchNorm2d
    int vec;                     // float4 path: P, chunk multiples of 4, tensors 16-B aligned
};

// The forward statistics from the channel's sums s1, s2 of (z - K), (z - K)^2: the only place that
// forms mean, variance and invstd
struct BnStat {
    float m32, is32;   // mean, 1 / sqrt(var + eps)
    double var;        // biased, clamped at 0
};
__device__ __forceinline__ BnStat bn_fwd_stat(const BnArgs &a, double K, double s1, double s2) {
    const double m = s1 / a.P;
    double var = s2 / a.P - m * m;
    if (var < 0.0) var = 0.0;
    return {(float)(K + m), (float)(1.0 / sqrt(var + (double)a.eps)), var};
}

// ... stored, with the running statistics' momentum update, by one thread per channel
__device__ __forceinline__ void bn_fwd_store(const BnArgs &a, int c, const BnStat &s) {
    a.mean[c] = s.m32;
    a.invstd[c] = s.is32;
    if (a.run_mean) {
        const double unb = a.P > 1 ? s.var * a.P / (a.P - 1) : s.var;
        a.run_mean[c] = (1.0f - a.momentum) * a.run_mean[c] + a.momentum * s.m32;
        a.run_var[c] = (1.0f - a.momentum) * a.run_var[c] + a.momentum * (float)unb;
    }
}

// The one-workgroup forms: every thread derives the statistics from the block sums, thread 0 stores them
__device__ __forceinline__ void bn_fwd_finish(const BnArgs &a, int c, double K, double s1, double s2, float &m32,
                                              float &is32) {
    const BnStat s = bn_fwd_stat(a, K, s1, s2);
    m32 = s.m32;
    is32 = s.is32;
    if (threadIdx.x == 0) bn_fwd_store(a, c, s);
}

// y = act(x_hat gm + bt) with x_hat = (z - mean) invstd: the forward's normalisation, every form's
__device__ __forceinline__ float bn_norm_act(float v, float m32, float is32, float gm, float bt, int act) {
    return act_fwd((v - m32) * is32 * gm + bt, act);
}
__device__ __forceinline__ float4 bn_norm_act(const float4 &v, float m32, float is32, float gm, float bt, int act) {
    return make_float4(bn_norm_act(v.x, m32, is32, gm, bt, act), bn_norm_act(v.y, m32, is32, gm, bt, act),
                       bn_norm_act(v.z, m32, is32, gm, bt, act), bn_norm_act(v.w, m32, is32, gm, bt, act));
}

// partial sums of (z - K), (z - K)^2 over this workgroup's slice, K = z[c][0] (stable variance);
// block-reduced (valid in every thread), both sums behind one barrier
__device__ __forceinline__ void bn_stats_body(const BnArgs &a, int c, int sb, double &s1, double &s2, double *red) {
    const float *z = a.z + (int64_t)c * a.P;
    const int i0 = sb * a.chunk, i1 = min(a.P, i0 + a.chunk);
    const double K = (double)z[0];
    s1 = 0.0;
    s2 = 0.0;
    if (a.vec) {   // one float4 per lane per pass: 16-B loads, 4x the bytes in flight
        const float4 *z4 = reinterpret_cast<const float4 *>(z);
        for (int q = (i0 >> 2) + threadIdx.x; q < (i1 >> 2); q += blockDim.x) {
            const float4 v = z4[q];
            const double d0 = (double)v.x - K, d1 = (double)v.y - K, d2 = (double)v.z - K, d3 = (double)v.w - K;
            s1 += d0; s2 += d0 * d0;
            s1 += d1; s2 += d1 * d1;
            s1 += d2; s2 += d2 * d2;
            s1 += d3; s2 += d3 * d3;
        }
    } else {
        for (int i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
            const double d = (double)z[i] - K;
            s1 += d;
            s2 += d * d;
        }
    }
    block_sum2_d(s1, s2, red);
}

__global__ __launch_bounds__(kBnThreads) void k_bn_stats(BnArgs a) {
    __shared__ double red[2 * kBnThreads / 64];
    const int c = blockIdx.y, sb = blockIdx.x;
    double s1, s2;
    bn_stats_body(a, c, sb, s1, s2, red);
    if (threadIdx.x == 0) {
        double *pp = a.part + ((int64_t)c * a.S + sb) * 3;
        pp[0] = s1;
        pp[1] = s2;
    }
}

// normalise + affine + activation of this workgroup's slice; t1, t2 = the channel's summed
// partials (read by thread 0 only).  ONE (k_bn_fwd1): t1, t2 valid in every thread, which then all
// form the statistics themselves (thread 0's arithmetic) and the Lipschitz scale per wave: no barrier
template <bool ONE = false>
__device__ __forceinline__ void bn_apply_body(const BnArgs &a, int c, int sb, double t1, double t2, float *redf,
                                              float *st_s) {
    const int64_t off = (int64_t)c * a.P;
    const float *z = a.z + off;
    float *y = a.y + off;
    const int i0 = sb * a.chunk, i1 = min(a.P, i0 + a.chunk);
    float cs, m32, is32;
    if constexpr (ONE) {
        cs = a.lip ? bn_lip_scale_w(a.gamma, a.C) : 1.0f;
        bn_fwd_finish(a, c, (double)a.z[off], t1, t2, m32, is32);
    } else {
        cs = a.lip ? bn_lip_scale(a.gamma, a.C, redf) : 1.0f;
        if (threadIdx.x == 0) {   // every workgroup of the channel broadcasts, its first one stores
            const BnStat s = bn_fwd_stat(a, (double)a.z[off], t1, t2);
            st_s[0] = s.m32;
            st_s[1] = s.is32;
            if (sb == 0) bn_fwd_store(a, c, s);
        }
        __syncthreads();
        m32 = st_s[0];
        is32 = st_s[1];
    }
    const float gm = a.gamma[c] / cs, bt = a.beta[c] / cs;
    if (a.vec) {
        const float4 *z4 = reinterpret_cast<const float4 *>(z);
        float4 *y4 = reinterpret_cast<float4 *>(y);
        for (int q = (i0 >> 2) + threadIdx.x; q < (i1 >> 2); q += blockDim.x) {
            const float4 v = z4[q];
            y4[q] = bn_norm_act(v, m32, is32, gm, bt, a.act);
        }
        return;
    }
    for (int i = i0 + threadIdx.x; i < i1; i += blockDim.x) y[i] = bn_norm_act(z[i], m32, is32, gm, bt, a.act);
}

__global__ __launch_bounds__(kBnThreads) void k_bn_apply(BnArgs a) {
    __shared__ float redf[kBnThreads / 64];
    __shared__ float st_s[2];
    const int c = blockIdx.y, sb = blockIdx.x;
    if (!a.bn) {
        const int64_t off = (int64_t)c * a.P;
        const int i0 = sb * a.chunk, i1 = min(a.P, i0 + a.chunk);
        for (int i = i0 + threadIdx.x; i < i1; i += blockDim.x) a.y[off + i] = act_fwd(a.z[off + i], a.act);
        return;
    }
    double t1 = 0.0, t2 = 0.0;
    if (threadIdx.x == 0) {
        const double *q = a.part + (int64_t)c * a.S * 3;
        for (int j = 0; j < a.S; ++j) { t1 += q[3 * j]; t2 += q[3 * j + 1]; }
    }
    bn_apply_body(a, c, sb, t1, t2, redf, st_s);
}

// S == 1 (a channel fits one workgroup): statistics and apply in one launch, the same
// arithmetic as k_bn_stats + k_bn_apply (0 + the single partial)
__global__ __launch_bounds__(kBn1Threads) void k_bn_fwd1(BnArgs a) {
    __shared__ double red[2 * kBn1Threads / 64];
    __shared__ float redf[kBn1Threads / 64];
    __shared__ float st_s[2];
    const int c = blockIdx.y;
    double s1, s2;
    bn_stats_body(a, c, 0, s1, s2, red);
    bn_apply_body<true>(a, c, 0, 0.0 + s1, 0.0 + s2, redf, st_s);
}

// Split-K finish + BatchNorm(+act) of one channel in one launch (a channel fits one workgroup:
// P <= 4 * kBn1Threads): z = sum of the GEMM's split-K partials (k_gemm_reduce's order) + bias,
// stored for the backward, then k_bn_fwd1's statistics / normalisation / activation from the
// values held in registers.  Replaces k_gemm_reduce + k_bn_fwd1 for the small-map convs.
template <int TH = kBn1Threads>
__global__ __launch_bounds__(TH) void k_reduce_bn1(const float *__restrict__ part, int nsplit,
                                                   const float *__restrict__ bias, BnArgs a,
                                                   const float *__restrict__ sdiv = nullptr) {
    __shared__ double red[2 * TH / 64];
    const int c = blockIdx.y, t = threadIdx.x;
    const int64_t MN = (int64_t)a.C * a.P, off = (int64_t)c * a.P;
    auto zsum = [&](int i) { return splitk_value1(part, nsplit, MN, off + i, sdiv, bias, c); };
    const float cs = a.lip ? bn_lip_scale_w(a.gamma, a.C) : 1.0f;
    float zv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = t + u * TH;
        zv[u] = 0.0f;
        if (i >= a.P) continue;
        zv[u] = zsum(i);
        const_cast<float *>(a.z)[off + i] = zv[u];
    }
    // K = z[c][0], formed again by every thread (the same sum, so the same value) instead of being
    // broadcast from thread 0 behind a barrier
    const double K = (double)zsum(0);
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (t + u * TH < a.P) {
            const double d = (double)zv[u] - K;
            s1 += d;
            s2 += d * d;
        }
    block_sum2_d(s1, s2, red);   // the only barrier
    float m32, is32;
    bn_fwd_finish(a, c, K, s1, s2, m32, is32);
    const float gm = a.gamma[c] / cs, bt = a.beta[c] / cs;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = t + u * TH;
        if (i < a.P) a.y[off + i] = bn_norm_act(zv[u], m32, is32, gm, bt, a.act);
    }
}

struct BnBwdArgs {
    const float *gy;             // [C][P] dL/dy
    const float *y, *z;          // activation output, conv output
    const float *gamma;          // bn gamma_orig (null when !bn)
    const float *mean, *invstd;
    float *gz;                   // [C][P] dL/dz (may alias gy)
    float *ggamma, *gbeta;       // [C] grads of gamma_orig / beta_orig (null when !bn)
    float *gbias;                // [C] grad of the conv bias = sum_p dL/dz
    double *part;                // [C][S][3] partials
    int C, P, S, chunk, bn, act;
    int lip;                     // BatchNormSpectralNorm rescale (1-Lip) or plain BatchNorm2d
    int accum;                   // gz += instead of gz =
    int vec;                     // float4 path: P, chunk multiples of 4, tensors 16-B aligned
    const float *beta;           // bn beta_orig: with it the LeakyReLU branch is taken from z (bn_act_bwd)
};

// dL/d(pre-activation) of a BN node: for LeakyReLU the branch is decided on pre = x_hat gm + bt, the
// forward's own arithmetic ((z - m) is) gm + bt, so y need not be read (same decisions bitwise: y > 0
// iff pre > 0); a Sigmoid (or no beta) takes y.
__device__ __forceinline__ bool bn_needs_y(const BnBwdArgs &a) { return a.act == LRS_ACT_SIGMOID || !a.beta; }
__device__ __forceinline__ float bn_act_bwd(float g, float xh, float gm, float bt, float y, const BnBwdArgs &a) {
    if (a.act == LRS_ACT_LRELU && a.beta) {
        const float pre = xh * gm + bt;
        return pre > 0.0f ? g : g * 0.2f;
    }
    return act_bwd(g, y, a.act);
}

// dL/dz of one element = k (g - mean(g) - x_hat mean(g x_hat)), k = gm invstd: the backward's output, every form's
__device__ __forceinline__ float bn_bwd_out(float k, float g, float xh, float mg, float mgx) {
    return k * (g - mg - xh * mgx);
}

// redf: the Lipschitz scale's reduction scratch (kBn*Threads / 64 floats); with beta the LeakyReLU
// branch comes from the pre-activation (bn_act_bwd), so y is not read.  The three sums behind one
// barrier (red >= 3 x blockDim / 64 doubles); ONE (k_bn_bwd1): the scale per wave (no barrier)
template <bool ONE = false>
__device__ __forceinline__ void bn_bwd_stats_body(const BnBwdArgs &a, int c, int sb, double (&o)[3], double *red,
                                                  float *redf) {
    const int64_t off = (int64_t)c * a.P;
    const float *gy = a.gy + off, *y = a.y + off, *z = a.z + off;
    const int i0 = sb * a.chunk, i1 = min(a.P, i0 + a.chunk);
    double sg = 0.0, sgx = 0.0, sx = 0.0;
    const bool ldy = bn_needs_y(a);
    float gm = 0.0f, bt = 0.0f;
    if (a.bn && !ldy) {
        float cs = 1.0f;
        if constexpr (ONE) cs = a.lip ? bn_lip_scale_w(a.gamma, a.C) : 1.0f;
        else cs = a.lip ? bn_lip_scale(a.gamma, a.C, redf) : 1.0f;
        gm = a.gamma[c] / cs;
        bt = a.beta[c] / cs;
    }
    if (a.bn && a.vec) {
        const float m32 = a.mean[c], is32 = a.invstd[c];
        const float4 *gy4 = reinterpret_cast<const float4 *>(gy), *y4 = reinterpret_cast<const float4 *>(y),
                     *z4 = reinterpret_cast<const float4 *>(z);
        for (int q = (i0 >> 2) + threadIdx.x; q < (i1 >> 2); q += blockDim.x) {
            const float4 gv = gy4[q], zv = z4[q];
            const float4 yv = ldy ? y4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float ge[4] = {gv.x, gv.y, gv.z, gv.w}, ye[4] = {yv.x, yv.y, yv.z, yv.w},
                        ze[4] = {zv.x, zv.y, zv.z, zv.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xh = (ze[e] - m32) * is32;
                const float g = ldy ? act_bwd(ge[e], ye[e], a.act) : bn_act_bwd(ge[e], xh, gm, bt, 0.0f, a);
                sg += (double)g;
                sgx += (double)g * (double)xh;
                sx += (double)xh;
            }
        }
    } else if (a.bn) {
        const float m32 = a.mean[c], is32 = a.invstd[c];
        for (int i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
            const float xh = (z[i] - m32) * is32;
            const float g = ldy ? act_bwd(gy[i], y[i], a.act) : bn_act_bwd(gy[i], xh, gm, bt, 0.0f, a);
            sg += (double)g;
            sgx += (double)g * (double)xh;
            sx += (double)xh;
        }
    } else {
        for (int i = i0 + threadIdx.x; i < i1; i += blockDim.x) sg += (double)act_bwd(gy[i], y[i], a.act);
    }
    block_sum3_d(sg, sgx, sx, red);
    o[0] = sg;
    o[1] = sgx;
    o[2] = sx;
}

__global__ __launch_bounds__(kBnThreads) void k_bn_bwd_stats(BnBwdArgs a) {
    __shared__ double red[3 * kBnThreads / 64];
    __shared__ float redf[kBnThreads / 64];
    const int c = blockIdx.y, sb = blockIdx.x;
    double o[3];
    bn_bwd_stats_body(a, c, sb, o, red, redf);
    if (threadIdx.x == 0) {
        double *pp = a.part + ((int64_t)c * a.S + sb) * 3;
        pp[0] = o[0];
        pp[1] = o[1];
        pp[2] = o[2];
    }
}

// t = the channel's summed partials (read by thread 0 only).  ONE (k_bn_bwd1): t valid in every
// thread, which then all form mean(g), mean(g x_hat) themselves and the scale per wave: no barrier
template <bool ONE = false>
__device__ __forceinline__ void bn_bwd_apply_body(const BnBwdArgs &a, int c, int sb, const double (&t)[3],
                                                  float *redf, float *st_s) {
    const int64_t off = (int64_t)c * a.P;
    const float *gy = a.gy + off, *y = a.y + off, *z = a.z + off;
    float *gz = a.gz + off;
    const int i0 = sb * a.chunk, i1 = min(a.P, i0 + a.chunk);
    if (!a.bn) {
        if (threadIdx.x == 0 && sb == 0 && a.gbias) a.gbias[c] = (float)t[0];
        for (int i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
            const float v = act_bwd(gy[i], y[i], a.act);
            gz[i] = a.accum ? gz[i] + v : v;
        }
        return;
    }
    float cs = 1.0f;
    if constexpr (ONE) cs = a.lip ? bn_lip_scale_w(a.gamma, a.C) : 1.0f;
    else cs = a.lip ? bn_lip_scale(a.gamma, a.C, redf) : 1.0f;
    const float m32 = a.mean[c], is32 = a.invstd[c];
    const float gm = a.gamma[c] / cs;
    const float k = gm * is32;
    const bool ldy = bn_needs_y(a);
    const float bt = ldy ? 0.0f : a.beta[c] / cs;
    float mg, mgx;
    if (ONE || threadIdx.x == 0) {
        mg = (float)(t[0] / a.P);
        mgx = (float)(t[1] / a.P);
        if (!ONE) {
            st_s[0] = mg;
            st_s[1] = mgx;
        }
        if (threadIdx.x == 0 && sb == 0) {
            a.ggamma[c] = (float)t[1] / cs;
            a.gbeta[c] = (float)t[0] / cs;
            // conv bias grad = sum_p gz = k (sg - P mg - mgx sum_p xhat)  (zero in exact arithmetic)
            if (a.gbias) a.gbias[c] = (float)((double)k * (t[0] - (double)a.P * mg - (double)mgx * t[2]));
        }
    }
    if constexpr (!ONE) {
        __syncthreads();
        mg = st_s[0];
        mgx = st_s[1];
    }
    if (a.vec) {
        const float4 *gy4 = reinterpret_cast<const float4 *>(gy), *y4 = reinterpret_cast<const float4 *>(y),
                     *z4 = reinterpret_cast<const float4 *>(z);
        float4 *gz4 = reinterpret_cast<float4 *>(gz);
        for (int q = (i0 >> 2) + threadIdx.x; q < (i1 >> 2); q += blockDim.x) {
            const float4 gv = gy4[q], zv = z4[q];
            const float4 yv = ldy ? y4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float ge[4] = {gv.x, gv.y, gv.z, gv.w}, ye[4] = {yv.x, yv.y, yv.z, yv.w},
                        ze[4] = {zv.x, zv.y, zv.z, zv.w};
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xh = (ze[e] - m32) * is32;
                const float g = ldy ? act_bwd(ge[e], ye[e], a.act) : bn_act_bwd(ge[e], xh, gm, bt, 0.0f, a);
                o[e] = bn_bwd_out(k, g, xh, mg, mgx);
            }
            float4 r = make_float4(o[0], o[1], o[2], o[3]);
            if (a.accum) {
                const float4 pv = gz4[q];
                r = make_float4(pv.x + r.x, pv.y + r.y, pv.z + r.z, pv.w + r.w);
            }
            gz4[q] = r;
        }
        return;
    }
    for (int i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
        const float xh = (z[i] - m32) * is32;
        const float g = ldy ? act_bwd(gy[i], y[i], a.act) : bn_act_bwd(gy[i], xh, gm, bt, 0.0f, a);
        const float v = bn_bwd_out(k, g, xh, mg, mgx);
        gz[i] = a.accum ? gz[i] + v : v;
    }
}

__global__ __launch_bounds__(kBnThreads) void k_bn_bwd_apply(BnBwdArgs a) {
    __shared__ float redf[kBnThreads / 64];
    __shared__ float st_s[2];
    const int c = blockIdx.y, sb = blockIdx.x;
    double t[3] = {0.0, 0.0, 0.0};
    if (threadIdx.x == 0 && (a.bn || (sb == 0 && a.gbias))) {
        const double *q = a.part + (int64_t)c * a.S * 3;
        for (int j = 0; j < a.S; ++j)
            for (int e = 0; e < 3; ++e) t[e] += q[3 * j + e];
    }
    bn_bwd_apply_body(a, c, sb, t, redf, st_s);
}

// S == 1: statistics and apply in one launch (same arithmetic as the two-kernel path)
__global__ __launch_bounds__(kBn1Threads) void k_bn_bwd1(BnBwdArgs a) {
    __shared__ double red[3 * kBn1Threads / 64];
    __shared__ float redf[kBn1Threads / 64];
    __shared__ float st_s[2];
    const int c = blockIdx.y;
    double o[3];
    bn_bwd_stats_body<true>(a, c, 0, o, red, redf);
    const double t[3] = {0.0 + o[0], 0.0 + o[1], 0.0 + o[2]};
    bn_bwd_apply_body<true>(a, c, 0, t, redf, st_s);
}

// ---- one workgroup per channel, the channel held in registers (P <= 4096 NQ, float4 path) ----
// For the mid-size maps (98^2, 196^2 in configs[2]) the two-launch S-way split (statistics, then
// apply, each re-reading the channel) costs more than one 1024-thread workgroup per channel that
// reads every value once: thread t holds the float4 quads t + 1024 u, u < NQ.  The statistics are
// the same fp64 shifted sums (K = z[c][0]) as k_bn_stats / k_bn_bwd_stats; only their summation
// order differs.
constexpr int kBnRegMaxQ = 10;   // 40960 pixels

template <int NQ>
__device__ __forceinline__ bool bnr_ok(int P, int u) { return threadIdx.x + u * kBn1Threads < (unsigned)(P >> 2); }

// quad q of a [C][P] tensor at channel offset off, summed over nsplit split-K partials (stride MN):
// acc[e] = the splits e, e + 8, ... in increasing order (k_gemm_reduce's order); the loads of one
// group of 8 are predicated, not indexed, so acc stays in registers
__device__ __forceinline__ float4 splitk_sum4(const float *__restrict__ part, int nsplit, int64_t MN, int64_t off, int q) {
    float4 acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int z0 = 0; z0 < nsplit; z0 += 8) {
        float4 p[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
            p[e] = z0 + e < nsplit ? reinterpret_cast<const float4 *>(part + (int64_t)(z0 + e) * MN + off)[q]
                                   : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (z0 + e < nsplit) {
                acc[e].x += p[e].x; acc[e].y += p[e].y; acc[e].z += p[e].z; acc[e].w += p[e].w;
            }
    }
    float4 v;
    v.x = ((acc[0].x + acc[1].x) + (acc[2].x + acc[3].x)) + ((acc[4].x + acc[5].x) + (acc[6].x + acc[7].x));
    v.y = ((acc[0].y + acc[1].y) + (acc[2].y + acc[3].y)) + ((acc[4].y + acc[5].y) + (acc[6].y + acc[7].y));
    v.z = ((acc[0].z + acc[1].z) + (acc[2].z + acc[3].z)) + ((acc[4].z + acc[5].z) + (acc[6].z + acc[7].z));
    v.w = ((acc[0].w + acc[1].w) + (acc[2].w + acc[3].w)) + ((acc[4].w + acc[5].w) + (acc[6].w + acc[7].w));
    return v;
}

// splitk_value1 for quad q of the channel at offset off
__device__ __forceinline__ float4 splitk_value4(const float *part, int nsplit, int64_t MN, int64_t off, int q,
                                                const float *sdiv, const float *bias, int c) {
    float4 v = splitk_sum4(part, nsplit, MN, off, q);
    if (sdiv) {
        const float sc = *sdiv;
        v.x = v.x / sc; v.y = v.y / sc; v.z = v.z / sc; v.w = v.w / sc;
    }
    if (bias) {
        const float b = bias[c];
        v.x = v.x + b; v.y = v.y + b; v.z = v.z + b; v.w = v.w + b;
    }
    return v;
}

// forward: z = (split-K partials summed in k_gemm_reduce's order + bias) or z as stored; then
// BN statistics, normalisation, affine (Lipschitz rescale), activation.  part == nullptr: z given.
// sdiv (nullable): the raw-weight conv's scale (splitk_value1).
template <int NQ>
__global__ __launch_bounds__(kBn1Threads) void k_bn_fwd_r(const float *__restrict__ part, int nsplit,
                                                 const float *__restrict__ bias, BnArgs a,
                                                 const float *__restrict__ sdiv = nullptr) {
    __shared__ double red[2 * kBn1Threads / 64];
    const int c = blockIdx.y, t = threadIdx.x;
    const int64_t MN = (int64_t)a.C * a.P, off = (int64_t)c * a.P;
    const float cs = a.lip ? bn_lip_scale_w(a.gamma, a.C) : 1.0f;
    float4 zv[NQ];
    float4 *z4 = reinterpret_cast<float4 *>(const_cast<float *>(a.z) + off);
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
        zv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!bnr_ok<NQ>(a.P, u)) continue;
        const int q = t + u * kBn1Threads;
        if (!part) {
            zv[u] = z4[q];
            continue;
        }
        float4 v = splitk_value4(part, nsplit, MN, off, q, sdiv, bias, c);
        zv[u] = v;
        z4[q] = v;
    }
    // K = z[c][0] (thread 0's first value), formed again by every thread: no broadcast barrier
    float k0;
    if (part) {
        k0 = splitk_value4(part, nsplit, MN, off, 0, sdiv, bias, c).x;
    } else {
        k0 = z4[0].x;
    }
    const double K = (double)k0;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int u = 0; u < NQ; ++u)
        if (bnr_ok<NQ>(a.P, u)) {
            const double d0 = (double)zv[u].x - K, d1 = (double)zv[u].y - K, d2 = (double)zv[u].z - K,
                         d3 = (double)zv[u].w - K;
            s1 += d0; s2 += d0 * d0;
            s1 += d1; s2 += d1 * d1;
            s1 += d2; s2 += d2 * d2;
            s1 += d3; s2 += d3 * d3;
        }
    block_sum2_d(s1, s2, red);   // the only barrier
    float m32, is32;
    bn_fwd_finish(a, c, K, s1, s2, m32, is32);
    const float gm = a.gamma[c] / cs, bt = a.beta[c] / cs;
    float4 *y4 = reinterpret_cast<float4 *>(a.y + off);
#pragma unroll
    for (int u = 0; u < NQ; ++u)
        if (bnr_ok<NQ>(a.P, u)) y4[t + u * kBn1Threads] = bn_norm_act(zv[u], m32, is32, gm, bt, a.act);
}

// Split-K finish + BatchNorm(+act) backward of one channel in one launch (P <= 4096: four values per
// thread, any P): dL/dy = the sum of the data-gradient GEMM's split-K partials (k_gemm_reduce's
// order; dL/dy itself is not stored: only this kernel reads it), then k_bn_bwd_r's arithmetic.
// Replaces k_gemm_reduce + k_bn_bwd1 below a small-map conv's data gradient.
template <int TH = kBn1Threads>
__global__ __launch_bounds__(TH) void k_reduce_bn_bwd1(const float *__restrict__ part, int nsplit, BnBwdArgs a) {
    __shared__ double red[3 * TH / 64];
    const int c = blockIdx.y, t = threadIdx.x;
    const int64_t MN = (int64_t)a.C * a.P, off = (int64_t)c * a.P;
    const float m32 = a.mean[c], is32 = a.invstd[c];
    const float cs = a.lip ? bn_lip_scale_w(a.gamma, a.C) : 1.0f;
    const float gm = a.gamma[c] / cs, bt = a.beta ? a.beta[c] / cs : 0.0f;
    const bool ldy = bn_needs_y(a);
    float g[4], xh[4];
    double sg = 0.0, sgx = 0.0, sx = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = t + u * TH;
        g[u] = xh[u] = 0.0f;
        if (i >= a.P) continue;
        const float gy = splitk_sum1(part, nsplit, MN, off + i);
        xh[u] = (a.z[off + i] - m32) * is32;
        g[u] = bn_act_bwd(gy, xh[u], gm, bt, ldy ? a.y[off + i] : 0.0f, a);
        sg += (double)g[u];
        sgx += (double)g[u] * (double)xh[u];
        sx += (double)xh[u];
    }
    block_sum3_d(sg, sgx, sx, red);   // the only barrier
    const float k = gm * is32;
    const float mg = (float)(sg / a.P), mgx = (float)(sgx / a.P);
    if (t == 0) {
        a.ggamma[c] = (float)sgx / cs;
        a.gbeta[c] = (float)sg / cs;
        if (a.gbias) a.gbias[c] = (float)((double)k * (sg - (double)a.P * mg - (double)mgx * sx));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = t + u * TH;
        if (i >= a.P) continue;
        const float v = bn_bwd_out(k, g[u], xh[u], mg, mgx);
        a.gz[off + i] = a.accum ? a.gz[off + i] + v : v;
    }
}

// backward (a.bn): g = act'(dL/dy) and x_hat held in registers, the three fp64 sums, then
// dL/dz = k (g - mean(g) - x_hat mean(g x_hat)) (+= when accumulating), and the parameter grads
template <int NQ>
__global__ __launch_bounds__(kBn1Threads) void k_bn_bwd_r(BnBwdArgs a) {
    __shared__ double red[3 * kBn1Threads / 64];
    const int c = blockIdx.y, t = threadIdx.x;
    const int64_t off = (int64_t)c * a.P;
    const float4 *gy4 = reinterpret_cast<const float4 *>(a.gy + off), *y4 = reinterpret_cast<const float4 *>(a.y + off),
                 *z4 = reinterpret_cast<const float4 *>(a.z + off);
    const float m32 = a.mean[c], is32 = a.invstd[c];
    const float cs = a.lip ? bn_lip_scale_w(a.gamma, a.C) : 1.0f;
    const float gm = a.gamma[c] / cs, bt = a.beta ? a.beta[c] / cs : 0.0f;
    const bool ldy = bn_needs_y(a);
    float g[NQ][4], xh[NQ][4];
    double sg = 0.0, sgx = 0.0, sx = 0.0;
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
#pragma unroll
        for (int e = 0; e < 4; ++e) g[u][e] = xh[u][e] = 0.0f;
        if (!bnr_ok<NQ>(a.P, u)) continue;
        const int q = t + u * kBn1Threads;
        const float4 gv = gy4[q], yv = ldy ? y4[q] : make_float4(0.f, 0.f, 0.f, 0.f), zv = z4[q];
        const float ge[4] = {gv.x, gv.y, gv.z, gv.w}, ye[4] = {yv.x, yv.y, yv.z, yv.w}, ze[4] = {zv.x, zv.y, zv.z, zv.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            xh[u][e] = (ze[e] - m32) * is32;
            g[u][e] = bn_act_bwd(ge[e], xh[u][e], gm, bt, ye[e], a);
            sg += (double)g[u][e];
            sgx += (double)g[u][e] * (double)xh[u][e];
            sx += (double)xh[u][e];
        }
    }
    block_sum3_d(sg, sgx, sx, red);   // the only barrier
    const float k = gm * is32;
    const float mg = (float)(sg / a.P), mgx = (float)(sgx / a.P);
    if (t == 0) {
        a.ggamma[c] = (float)sgx / cs;
        a.gbeta[c] = (float)sg / cs;
        if (a.gbias) a.gbias[c] = (float)((double)k * (sg - (double)a.P * mg - (double)mgx * sx));
    }
    float4 *gz4 = reinterpret_cast<float4 *>(a.gz + off);
#pragma unroll
    for (int u = 0; u < NQ; ++u)
        if (bnr_ok<NQ>(a.P, u)) {
            const int q = t + u * kBn1Threads;
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = bn_bwd_out(k, g[u][e], xh[u][e], mg, mgx);
            float4 r = make_float4(o[0], o[1], o[2], o[3]);
            if (a.accum) {
                const float4 pv = gz4[q];
                r = make_float4(pv.x + r.x, pv.y + r.y, pv.z + r.z, pv.w + r.w);
            }
            gz4[q] = r;
        }
}

// ==========================================================================================
// Host: which form serves a shape, and the launches that depend on it
// ==========================================================================================

// workgroups per channel for the BN kernels: ~4096 elements each, at most 64
inline int bn_split(int64_t P) {
    int64_t S = (P + 4095) / 4096;
    if (S < 1) S = 1;
    if (S > 64) S = 64;
    return (int)S;
}

inline int64_t bn_part_doubles(int C, int64_t P) { return (int64_t)C * bn_split(P) * 3; }

// a BatchNorm channel that fits one workgroup: k_reduce_bn1 / k_reduce_bn_bwd1 can finish a pending
// split-K sum themselves
inline bool bn_one_wg(int64_t P) { return P <= 4 * kBn1Threads && bn_split(P) == 1; }

// Register-resident one-workgroup-per-channel BN (k_bn_fwd_r / k_bn_bwd_r): float4 quads per
// thread for a channel of P pixels, or 0 where the S-way split / the P <= 4096 kernels are used.
inline int bn_reg_q(int64_t P, bool vec) {
    if (!vec || P <= 4 * kBn1Threads || P > (int64_t)4 * kBn1Threads * kBnRegMaxQ) return 0;
    const int q = (int)((P + 4 * kBn1Threads - 1) / (4 * kBn1Threads));
    static const int qs[] = {2, 3, 4, 6, 8, 10};
    for (int v : qs)
        if (v >= q) return v;
    return 0;
}

// Threads of a one-workgroup-per-channel BatchNorm kernel (k_reduce_bn1, k_reduce_bn_bwd1, k_bn_fwd1,
// k_bn_bwd1): kBn1Small where the channel fits 2 values per thread of it (the 18^2 and smaller maps at
// 36^2, the 13^2 ones at 196^2), else kBn1Threads.  A/B (2 interleaved rounds): 36^2 step 0.671 ->
// 0.657 ms with 256 threads up to 1024 pixels, but the 196^2 step 1.274 -> 1.280 (its 25^2 maps then
// hold 3 values per thread).  (A kBn1Small-thread kernel covers at most 4 values per thread.)
constexpr int64_t kBn1SmallMaxP = 2 * kBn1Small;
static_assert(kBn1SmallMaxP <= 4 * kBn1Small, "a kBn1Small-thread kernel holds 4 values per thread");
inline int bn1_threads(int64_t P) { return P <= kBn1SmallMaxP ? kBn1Small : kBn1Threads; }

// The register form for nq = bn_reg_q(P, vec) > 0, one 1024-thread workgroup per channel.  The callers
// check the launch.
#define LRS_BNR_SWITCH(nq, K, ...)                                                                \
    switch (nq) {                                                                                 \
    case 2: hipLaunchKernelGGL(K<2>, __VA_ARGS__); break;                                         \
    case 3: hipLaunchKernelGGL(K<3>, __VA_ARGS__); break;                                         \
    case 4: hipLaunchKernelGGL(K<4>, __VA_ARGS__); break;                                         \
    case 6: hipLaunchKernelGGL(K<6>, __VA_ARGS__); break;                                         \
    case 8: hipLaunchKernelGGL(K<8>, __VA_ARGS__); break;                                         \
    default: hipLaunchKernelGGL(K<10>, __VA_ARGS__); break;                                       \
    }

// part (nullable): the product's nsplit split-K partials, finished with bias and sdiv (k_bn_fwd_r)
inline void launch_bn_fwd_r(int nq, const float *part, int nsplit, const float *bias, const BnArgs &a,
                            const float *sdiv, hipStream_t st) {
    LRS_BNR_SWITCH(nq, k_bn_fwd_r, dim3(1, a.C), dim3(kBn1Threads), 0, st, part, nsplit, bias, a, sdiv);
}

inline void launch_bn_bwd_r(int nq, const BnBwdArgs &a, hipStream_t st) {
    LRS_BNR_SWITCH(nq, k_bn_bwd_r, dim3(1, a.C), dim3(kBn1Threads), 0, st, a);
}
#undef LRS_BNR_SWITCH

// The one-workgroup forms that finish a split-K sum (bn_one_wg(a.P)), on bn1_threads(a.P) threads
inline void launch_reduce_bn1(const float *part, int nsplit, const float *bias, const BnArgs &a, const float *sdiv,
                              hipStream_t st) {
    if (bn1_threads(a.P) == kBn1Small)
        hipLaunchKernelGGL(k_reduce_bn1<kBn1Small>, dim3(1, a.C), dim3(kBn1Small), 0, st, part, nsplit, bias, a, sdiv);
    else
        hipLaunchKernelGGL(k_reduce_bn1<kBn1Threads>, dim3(1, a.C), dim3(kBn1Threads), 0, st, part, nsplit, bias, a,
                           sdiv);
}

inline void launch_reduce_bn_bwd1(const float *part, int nsplit, const BnBwdArgs &a, hipStream_t st) {
    if (bn1_threads(a.P) == kBn1Small)
        hipLaunchKernelGGL(k_reduce_bn_bwd1<kBn1Small>, dim3(1, a.C), dim3(kBn1Small), 0, st, part, nsplit, a);
    else
        hipLaunchKernelGGL(k_reduce_bn_bwd1<kBn1Threads>, dim3(1, a.C), dim3(kBn1Threads), 0, st, part, nsplit, a);
}

}  // namespace lrs

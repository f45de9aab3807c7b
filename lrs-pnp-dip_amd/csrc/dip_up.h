// DIP low-rank prox, the Deep Decoder stage's own kernels (LRS_NODE_DECODE): bilinear x2 upsampling fused
// with the stage's activation, forward and backward, and the activation alone for the stage that does not
// upsample.  Reference: include/decoder.py decodernw -- conv 1x1 (no bias) -> nn.Upsample(scale_factor=2,
// mode='bilinear') -> act_fun -> BatchNorm2d.  Part of dipnet.hip's translation unit.
//
// nn.Upsample(x2, bilinear, align_corners=False): output o = 2 s + p (p = 0, 1) samples the source at
// s + p / 2 - 1 / 4, i.e. 3/4 of source s and 1/4 of its neighbour s - 1 (p = 0) or s + 1 (p = 1), the
// neighbour's index clamped to the map.  In two dimensions the four weights are 9/16, 3/16, 3/16, 1/16.
#pragma once
#include "dip_kernels.h"

namespace lrs {

// the decoder stage's activations (NONE, LeakyReLU(0.2), ReLU); the derivative is taken from the sign of
// the stored activation a: both preserve the sign of the pre-activation, and a = 0 takes the slope of
// z <= 0 (ReLU: 0, LeakyReLU: 0.2), as torch does
__device__ __forceinline__ float dec_act_fwd(float v, int act) {
    if (act == LRS_ACT_RELU) return v > 0.0f ? v : 0.0f;
    if (act == LRS_ACT_LRELU) return v > 0.0f ? v : v * 0.2f;
    return v;
}
__device__ __forceinline__ float dec_act_bwd(float g, float a, int act) {
    if (act == LRS_ACT_RELU) return a > 0.0f ? g : 0.0f;
    if (act == LRS_ACT_LRELU) return a > 0.0f ? g : g * 0.2f;
    return g;
}

// One output value from its nearest source c, the two edge neighbours e0 / e1 and the diagonal d.  The
// chain starts at the smallest weight: with all four equal (every tap clamped) the partial sums are x/16,
// x/4 (exact), rn(7x/16) and rn(x + delta), |delta| <= ulp(x)/4: the input itself, bit for bit.
__device__ __forceinline__ float up2_tap(float c, float e0, float e1, float d) {
    return __builtin_fmaf(0.5625f, c, __builtin_fmaf(0.1875f, e0, __builtin_fmaf(0.1875f, e1, 0.0625f * d)));
}

// a[c][2H][2W] = act(up2(z[c][H][W])).  Block (bx, 256 / bx), grid (column pairs / bx, rows / by, C):
// thread (j, sy) reads the 3 x 4 source neighbourhood of source pixels (sy, 2j) and (sy, 2j + 1) (clamped
// indices, served by the cache: the source is 1/4 of the output) and writes the 2 x 4 output block at
// (2 sy, 4 j): two 16-byte stores when vec (W even, a 16-byte aligned), scalar stores otherwise.
__global__ __launch_bounds__(256) void k_up2_bilinear_act(const float *__restrict__ z, float *__restrict__ a, int H,
                                                          int W, int act, int vec) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, sy = blockIdx.y * blockDim.y + threadIdx.y;
    const int sx = 2 * j;
    if (sy >= H || sx >= W) return;
    const float *zc = z + (int64_t)blockIdx.z * H * W;
    const int ry[3] = {max(sy - 1, 0), sy, min(sy + 1, H - 1)};
    const int cx[4] = {max(sx - 1, 0), sx, min(sx + 1, W - 1), min(sx + 2, W - 1)};
    float v[3][4];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) v[r][q] = zc[ry[r] * W + cx[q]];
    const int Wo = 2 * W;
    float *ao = a + (int64_t)blockIdx.z * 4 * H * W + (int64_t)(2 * sy) * Wo + 2 * sx;
#pragma unroll
    for (int py = 0; py < 2; ++py) {
        const int nr = py ? 2 : 0;   // the neighbour row: above for the even output row, below for the odd one
        float o[4];
        // output column 4 j + q: nearest source column (cc) and its neighbour (nc) in v's columns
        o[0] = up2_tap(v[1][1], v[1][0], v[nr][1], v[nr][0]);
        o[1] = up2_tap(v[1][1], v[1][2], v[nr][1], v[nr][2]);
        o[2] = up2_tap(v[1][2], v[1][1], v[nr][2], v[nr][1]);
        o[3] = up2_tap(v[1][2], v[1][3], v[nr][2], v[nr][3]);
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = dec_act_fwd(o[q], act);
        float *row = ao + py * Wo;
        if (vec) {
            *reinterpret_cast<float4 *>(row) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
            row[0] = o[0];
            row[1] = o[1];
            if (sx + 1 < W) {
                row[2] = o[2];
                row[3] = o[3];
            }
        }
    }
}

// gz[c][H][W] = up2^T(ga .* act'(a)), ga and a [c][2H][2W]: a gather, no atomics.  Source row r is read by
// the output rows 2r - 1, 2r, 2r + 1, 2r + 2 with weights 1/4, 3/4, 3/4, 1/4; a row index outside the map is
// clamped, which folds the weight of the clamped tap onto the edge row (the forward's clamp, transposed).
// Columns alike.  Thread (j, sy) owns source pixels (sy, 2j) and (sy, 2j + 1): 4 rows x 6 columns of ga and a,
// summed in a fixed order (columns, then rows).  vec (W even, ga / a 16-byte aligned): the four centre
// columns of a row as one 16-byte load.
__global__ __launch_bounds__(256) void k_up2_bilinear_act_bwd(const float *__restrict__ ga, const float *__restrict__ a,
                                                              float *__restrict__ gz, int H, int W, int act, int vec) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, sy = blockIdx.y * blockDim.y + threadIdx.y;
    const int sx = 2 * j;
    if (sy >= H || sx >= W) return;
    const int Ho = 2 * H, Wo = 2 * W;
    const int64_t plane = (int64_t)blockIdx.z * Ho * Wo;
    const float *gc = ga + plane, *ac = a + plane;
    int cx[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) cx[q] = min(max(2 * sx - 1 + q, 0), Wo - 1);
    float h0[4], h1[4];   // per output row: the column sums of the two source pixels
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int oy = min(max(2 * sy - 1 + r, 0), Ho - 1);
        const float *gr = gc + (int64_t)oy * Wo, *ar = ac + (int64_t)oy * Wo;
        float g[6], y[6];
        if (vec) {
            const float4 g4 = *reinterpret_cast<const float4 *>(gr + 2 * sx), a4 = *reinterpret_cast<const float4 *>(ar + 2 * sx);
            g[0] = gr[cx[0]]; g[1] = g4.x; g[2] = g4.y; g[3] = g4.z; g[4] = g4.w; g[5] = gr[cx[5]];
            y[0] = ar[cx[0]]; y[1] = a4.x; y[2] = a4.y; y[3] = a4.z; y[4] = a4.w; y[5] = ar[cx[5]];
        } else {
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                g[q] = gr[cx[q]];
                y[q] = ar[cx[q]];
            }
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) g[q] = dec_act_bwd(g[q], y[q], act);
        h0[r] = ((0.25f * g[0] + 0.75f * g[1]) + 0.75f * g[2]) + 0.25f * g[3];
        h1[r] = ((0.25f * g[2] + 0.75f * g[3]) + 0.75f * g[4]) + 0.25f * g[5];
    }
    const float s0 = ((0.25f * h0[0] + 0.75f * h0[1]) + 0.75f * h0[2]) + 0.25f * h0[3];
    const float s1 = ((0.25f * h1[0] + 0.75f * h1[1]) + 0.75f * h1[2]) + 0.25f * h1[3];
    float *out = gz + (int64_t)blockIdx.z * H * W + (int64_t)sy * W + sx;
    out[0] = s0;
    if (sx + 1 < W) out[1] = s1;
}

// the stage without upsampling: a = act(z), and gz = ga .* act'(a), over n elements (float4 where vec)
__global__ __launch_bounds__(256) void k_dec_act(const float *__restrict__ z, float *__restrict__ a, int64_t n, int act,
                                                 int vec) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n4 = vec ? n / 4 : 0;
    for (int64_t q = t0; q < n4; q += stride) {
        float4 v = reinterpret_cast<const float4 *>(z)[q];
        v.x = dec_act_fwd(v.x, act); v.y = dec_act_fwd(v.y, act); v.z = dec_act_fwd(v.z, act); v.w = dec_act_fwd(v.w, act);
        reinterpret_cast<float4 *>(a)[q] = v;
    }
    for (int64_t i = 4 * n4 + t0; i < n; i += stride) a[i] = dec_act_fwd(z[i], act);
}

__global__ __launch_bounds__(256) void k_dec_act_bwd(const float *__restrict__ ga, const float *__restrict__ a,
                                                     float *__restrict__ gz, int64_t n, int act, int vec) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n4 = vec ? n / 4 : 0;
    for (int64_t q = t0; q < n4; q += stride) {
        const float4 g = reinterpret_cast<const float4 *>(ga)[q], y = reinterpret_cast<const float4 *>(a)[q];
        reinterpret_cast<float4 *>(gz)[q] = make_float4(dec_act_bwd(g.x, y.x, act), dec_act_bwd(g.y, y.y, act),
                                                        dec_act_bwd(g.z, y.z, act), dec_act_bwd(g.w, y.w, act));
    }
    for (int64_t i = 4 * n4 + t0; i < n; i += stride) gz[i] = dec_act_bwd(ga[i], a[i], act);
}

}  // namespace lrs

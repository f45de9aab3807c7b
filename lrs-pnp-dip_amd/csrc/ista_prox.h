// The ISTA prox of one gradient row in LDS, shared by the row-split (ista_rs.hip) and per-pattern
// Gram (ista_pat.hip) kernels: the skimage fast NLM chunk, the MATLAB NLmeansfilter point, the
// soft threshold's quotient and the LDS row swizzle both kernels use; and the arithmetic of the stages the two
// kernels have in common, as pure functions of values: the 4-MFMA chain, the FISTA rule, the gradient row,
// the coefs write, the image resource.  Loops, LDS and global addressing and barriers stay in the kernels.
// profiles/ista_stages/notes.txt records, form by form, which of these left every kernel's code as it was.
#pragma once
#include "lrs_common.h"
#include "lrs_nlm.h"

namespace lrs {

// numpy 'reflect' (no edge repeat) of index i into [0, K)
__device__ __forceinline__ int reflect_idx(int i, int K) {
    if (K == 1) return 0;
    const int period = 2 * (K - 1);
    i %= period;
    if (i < 0) i += period;
    return i >= K ? period - i : i;
}

// MATLAB 'symmetric' padding (edge repeated) of index i, |overhang| <= K
__device__ __forceinline__ int symmetric_idx(int i, int K) {
    if (i < 0) return -i - 1;
    if (i >= K) return 2 * K - 1 - i;
    return i;
}

// skimage 0.18.3 fast NLM of atoms a0..a0+3 of one gradient row in LDS
// gradient-row chunk index XOR-swizzled by block: [16 blocks][KP] floats read by the prox
__device__ __forceinline__ int gsw(int b, int a) { return a ^ ((b & 15) << 2); }

// The same chunk with the interior window (a0 - 3 .. a0 + 7 inside [0, K)) read as three aligned
// 16-byte LDS loads (the swizzle keeps 4-float groups contiguous); identical values and outputs.
__device__ __forceinline__ void prox_nlm_chunk_v4(const float *row, int b, int a0, int K, double kneg, double c0,
                                                  double seven, float (&out)[4]) {
    double w[11];
    if (a0 >= 4 && a0 + 8 <= K) {
        float4 v[3];
#pragma unroll
        for (int u = 0; u < 3; ++u) v[u] = *reinterpret_cast<const float4 *>(&row[gsw(b, a0 - 4 + 4 * u)]);
        const float f[12] = {v[0].x, v[0].y, v[0].z, v[0].w, v[1].x, v[1].y, v[1].z, v[1].w,
                             v[2].x, v[2].y, v[2].z, v[2].w};
#pragma unroll
        for (int k = 0; k < 11; ++k) w[k] = (double)f[k + 1];
    } else {
#pragma unroll
        for (int k = 0; k < 11; ++k) w[k] = (double)row[gsw(b, reflect_idx(a0 - 3 + k, K))];
    }
    int W1[7], W2[7], W3[7];
    nlm_weights<true>(w, kneg, W1, W2, W3);
    nlm_outputs<2>(w, W1, W2, W3, c0, seven, out);
}

__device__ __forceinline__ void prox_nlm_chunk(const float *row, int b, int a0, int K, double kneg, double c0,
                                               double seven, float (&out)[4]) {
    double w[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) w[k] = (double)row[gsw(b, reflect_idx(a0 - 3 + k, K))];
    int W1[7], W2[7], W3[7];
    nlm_weights<true>(w, kneg, W1, W2, W3);
    nlm_outputs<2>(w, W1, W2, W3, c0, seven, out);
}

// NLmeansfilter(g, 3, 3, h) of LRS-PnP(Matlab Code)/NLmeansfilter.m:18-78, one output, fp64, in the
// evaluation order of oracle/nlm_oracle.c:oracle_nlm_matlab_col
__device__ __forceinline__ float prox_nlm_matlab_point(const float *row, int b, int i, int K,
                                                       const double (&krow)[7], double h2) {
    double v[13];   // g-hat[i-6 .. i+6]
#pragma unroll
    for (int k = 0; k < 13; ++k) {
        const int j = i - 6 + k;
        v[k] = (j >= -3 && j < K + 3) ? (double)row[gsw(b, symmetric_idx(j, K))] : 0.0;
    }
    double sw = 0.0, av = 0.0, wmax = 0.0;
#pragma unroll
    for (int t = -3; t <= 3; ++t) {
        const int r = i + t;
        if (t == 0 || r < 0 || r >= K) continue;
        double d = 0.0;
#pragma unroll
        for (int u = -3; u <= 3; ++u) {
            const double df = v[6 + u] - v[6 + t + u];
            d = d + krow[u + 3] * (df * df);
        }
        const double wt = exp(-d / h2);
        if (wt > wmax) wmax = wt;
        sw = sw + wt;
        av = av + wt * v[6 + t];
    }
    av = av + wmax * v[6];
    sw = sw + wmax;
    return sw > 0.0 ? (float)(av / sw) : row[gsw(b, i)];
}

__device__ __forceinline__ void nlm_matlab_krow_d(double (&krow)[7]) {
#pragma unroll
    for (int u = -3; u <= 3; ++u) {
        const int a = u < 0 ? -u : u;
        double s = 0.0;
        for (int d = (a < 1 ? 1 : a); d <= 3; ++d) s = s + 1.0 / (double)(2 * d + 1);
        krow[u + 3] = s / 3.0;
    }
}

// acc + sum_e a[e] r[e] on v_mfma_f32_16x16x4_f32, e in order (r: float[4] or floatx4 in registers): b, D x
// and Q x in both kernels and k_ista_pat's Phi.  Not through it: k_ista_rs's D^T r (two chains interleaved
// pairwise in row_tile) and its Phi epilogue (written out there)
template <class R>
__device__ __forceinline__ floatx4 mfma_chain(floatx4 acc, float4 a, const R &r) {
    acc = mfma16x16x4(a.x, r[0], acc);
    acc = mfma16x16x4(a.y, r[1], acc);
    acc = mfma16x16x4(a.z, r[2], acc);
    acc = mfma16x16x4(a.w, r[3], acc);
    return acc;
}

// FISTA (lrs_ista_opts.accel), the rule both kernels follow, wave-uniform:
//   t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2 in fp64, beta_k = (t_k - 1) / t_{k+1} rounded once to float32,
//   and iteration `it` of Nit extrapolates unless it is the first (beta_1 = 0, so x_{k-1} needs no start
//   value) or the last (which leaves x_Nit itself for the outputs).
__device__ __forceinline__ double fista_tnext(double tk) { return 0.5 * (1.0 + sqrt(1.0 + 4.0 * tk * tk)); }
__device__ __forceinline__ float fista_beta(double tk, double tn) { return (float)((tk - 1.0) / tn); }
__device__ __forceinline__ bool fista_mom(int it, int Nit) { return it > 0 && it + 1 < Nit; }

// z_{k+1} = x_k + beta (x_k - x_{k-1}) of one atom tile
__device__ __forceinline__ floatx4 fista_extrapolate(floatx4 xn, floatx4 xold, float beta) { return xn + beta * (xn - xold); }

// a / b from y = 1/b (correctly rounded reciprocal) and one remainder step: the IEEE quotient
// away from overflow / underflow (…1-LiP.py:190 torch division by alpha)
__device__ __forceinline__ float rs_div(float a, float b, float y) {
    const float q = a * y;
    const float r = __fmaf_rn(-b, q, a);
    return __fmaf_rn(r, y, q);
}

// g = x + num / alpha of one atom tile: the lane's 4 atoms of its gradient row
__device__ __forceinline__ float4 ista_grad4(floatx4 xo, floatx4 num, float al, float ral) {
    float4 gr;
    gr.x = xo[0] + rs_div(num[0], al, ral);
    gr.y = xo[1] + rs_div(num[1], al, ral);
    gr.z = xo[2] + rs_div(num[2], al, ral);
    gr.w = xo[3] + rs_div(num[3], al, ral);
    return gr;
}

// atoms a0 .. a0 + 3 (below K) of one block's coefficient row
__device__ __forceinline__ void ista_coefs4(float *row, int a0, int K, floatx4 xv) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (a0 + e < K) row[a0 + e] = xv[e];
}

// A fragment-ordered image of `bytes` bytes as a buffer resource (raw loads, bounds-checked against bytes)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t ista_image(const float4 *img, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void *)img, 0, bytes, 0x00020000);
}

}  // namespace lrs

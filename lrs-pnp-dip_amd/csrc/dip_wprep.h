// Per-step weight preparation of the DIP engine's convs: W / scale and the pre-split bf16 planes the
// split-bf16 conv products read (dip_gemm.h LdPre, dip_sm.h SmPre, dip_pw.h).
#pragma once

#include "lrs_dip.h"
#include "lrs_split.h"

namespace lrs {

// Per-step weight preparation of every conv of a network in ONE launch (grid (blocks, convs)):
// Wn = W_bar / scale[si] for the spectrally normalised convs (lipschitz_constraint_layer.py:42-44)
// and the bf16 planes the split-bf16 kernels read, from the same W / scale quotient:
//   WF[p][co][kyx * Cp + ci]            forward operand (Cp = Cin rounded up to 16)
//   WD[p][ci][kyx * Cop + co]           data-gradient operand (W^T, Cop = Cout rounded up to 16), or,
//                                       for an upsampled stride-1 conv (ke > 0),
//   WE[p][ci][(ey * ke + ex) * Cop + co] the effective ke x ke kernel of its data gradient as a
//                                       stride-2 conv over dL/dz (dgrad_effective): the sum of the taps
//                                       W[a + k-1-ey][b + k-1-ex] over the 2 x 2 upsample children a, b
//   upc: an upsampled reflection-padded 3 x 3 conv run by output parity class (LdUpFwdTM /
//   LdUpDgradTM): instead of WF / WD,
//   WUF[p][cls][co][e * Cp + ci]         the class's 2 x 2 effective weights (e = 2 ey + ex, the sum
//                                        of W[co][ci][ky][kx] over ky in T(i, ey), kx in T(j, ex))
//   WUD[p][ci][(4 cls + e) * Cop + co]   the same, transposed, all classes (the data gradient's K)
// (the planes' element counts: wprep_elems, dip_launch.h)
struct ConvPrep {
    const float *W;
    float *Wn;          // nullable
    __bf16 *wf, *wd;    // nullable (wd holds WE when ke > 0)
    int Cout, Cin, kk, Cp, Cop, si, k, ke;   // si: scale index, -1 = no spectral norm
    int upc;
};

// effective weight of parity class (i, j), tap (ey, ex): the taps T(i, ey) x T(j, ex) summed in
// increasing ky, kx order (w = the 3 x 3 taps of one (co, ci))
__device__ __forceinline__ float upc_weight(const float *w, int i, int j, int ey, int ex) {
    const int y0 = (i == 0) ? (ey == 0 ? 0 : 1) : (ey == 0 ? 0 : 2), y1 = (i == 0) ? (ey == 0 ? 0 : 2) : (ey == 0 ? 1 : 2);
    const int x0 = (j == 0) ? (ex == 0 ? 0 : 1) : (ex == 0 ? 0 : 2), x1 = (j == 0) ? (ex == 0 ? 0 : 2) : (ex == 0 ? 1 : 2);
    float s = 0.0f;
    for (int ky = y0; ky <= y1; ++ky)
        for (int kx = x0; kx <= x1; ++kx) s = s + w[ky * 3 + kx];
    return s;
}

__device__ __forceinline__ void conv_prep_body(const ConvPrep &c, float s, int64_t i0, int64_t stride) {
    const int64_t nw = (int64_t)c.Cout * c.Cin * c.kk;
    if (c.Wn)
        for (int64_t i = i0; i < nw; i += stride) c.Wn[i] = c.W[i] / s;
    const int ed = c.upc ? 16 : (c.ke > 0 ? c.ke * c.ke : c.kk);
    // 32-bit index arithmetic (lrs_dipnet_create and the lrs_conv2d_* entry points reject a conv whose
    // planes reach 2^31 / 3 elements)
    const int nf = c.wf ? c.Cout * (c.upc ? 16 : c.kk) * c.Cp : 0, nd = c.wd ? c.Cin * ed * c.Cop : 0;
    auto put = [&](__bf16 *dst, int plane, int j, float x) {
        const Bf16Split q = split_bf16(x);
        dst[j] = q.b0;
        dst[plane + j] = q.b1;
        dst[2 * plane + j] = q.b2;
    };
    // forward planes (ci fastest: the W reads of a wave are kk floats apart)
    for (int i = (int)i0; i < nf; i += (int)stride) {
        float x = 0.0f;
        if (c.upc) {   // [cls][co][e * Cp + ci]
            const int cl = i / (c.Cout * 4 * c.Cp), rem = i - cl * c.Cout * 4 * c.Cp;
            const int co = rem / (4 * c.Cp), r = rem - co * 4 * c.Cp, e = r / c.Cp, ci = r - e * c.Cp;
            if (ci < c.Cin) {
                x = upc_weight(c.W + ((int64_t)co * c.Cin + ci) * 9, cl >> 1, cl & 1, e >> 1, e & 1);
                if (c.si >= 0) x = x / s;
            }
        } else {       // [co][kyx * Cp + ci]
            const int co = i / (c.kk * c.Cp), rem = i - co * c.kk * c.Cp, kyx = rem / c.Cp, ci = rem - kyx * c.Cp;
            if (ci < c.Cin) {
                x = c.W[((int64_t)co * c.Cin + ci) * c.kk + kyx];
                if (c.si >= 0) x = x / s;
            }
        }
        put(c.wf, nf, i, x);
    }
    // data-gradient planes [ci][e * Cop + co] (W^T): a wave covers 8 ci x 8 co of one e, so its W reads
    // touch 8 rows of W instead of 64 (co fastest alone put the lanes Cin kk floats apart)
    const int nci8 = (c.Cin + 7) / 8, ncob = c.Cop / 8, ndt = c.wd ? nci8 * 64 * ed * ncob : 0;
    for (int t = (int)i0; t < ndt; t += (int)stride) {
        const int l = t & 63, r = t >> 6;
        const int cob = r % ncob, r2 = r / ncob, e = r2 % ed, cib = r2 / ed;
        const int ci = 8 * cib + (l >> 3), co = 8 * cob + (l & 7);
        if (ci >= c.Cin) continue;
        float x = 0.0f;
        if (co < c.Cout) {
            const float *w = c.W + ((int64_t)co * c.Cin + ci) * c.kk;
            if (c.upc) {   // e = 4 cls + tap
                x = upc_weight(w, (e >> 2) >> 1, (e >> 2) & 1, (e & 3) >> 1, e & 1);
            } else if (c.ke > 0) {
                const int ey = e / c.ke, ex = e - ey * c.ke;
                for (int a = 0; a < 2; ++a)
                    for (int b = 0; b < 2; ++b) {
                        const int ky = a + c.k - 1 - ey, kx = b + c.k - 1 - ex;
                        if (ky >= 0 && ky < c.k && kx >= 0 && kx < c.k) x = x + w[ky * c.k + kx];
                    }
            } else {
                x = w[e];
            }
            if (c.si >= 0) x = x / s;
        }
        put(c.wd, nd, (ci * ed + e) * c.Cop + co, x);
    }
}

__global__ __launch_bounds__(256) void k_conv_prep(const ConvPrep *__restrict__ tab, const float *__restrict__ scale,
                                                   double *loss_acc, int *step) {
    if (loss_acc && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {   // a training step begins
        *loss_acc = 0.0;
        *step += 1;
    }
    const ConvPrep c = tab[blockIdx.y];
    conv_prep_body(c, c.si >= 0 ? scale[c.si] : 1.0f, (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                   (int64_t)gridDim.x * blockDim.x);
}

// one conv, no spectral norm (the standalone lrs_conv2d_* entry points)
__global__ __launch_bounds__(256) void k_conv_prep1(ConvPrep c) {
    conv_prep_body(c, 1.0f, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

}  // namespace lrs

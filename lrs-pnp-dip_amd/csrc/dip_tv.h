// DIP low-rank prox, a smoothness term on the net's output for a TV-regularised loss: anisotropic spatial
// TV, band TV and spatial-spectral TV (SSTV) of the image o[C][H][W] inside the output, its value and its
// gradient (lrs_sstv_f32).  With N = n_mean, phi(d) = sqrt(d^2 + eps^2) (|d| for eps = 0):
//   R(o) = (w_sp / N) sum [ phi(o[c,y+1,x] - o[c,y,x]) + phi(o[c,y,x+1] - o[c,y,x]) ]
//        + (w_bd / N) sum   phi(o[c+1,y,x] - o[c,y,x])
//        + (w_ss / N) sum [ phi(Dy Dc o) + phi(Dx Dc o) ],
//   Dy Dc o[c,y,x] = (o[c+1,y+1,x] - o[c,y+1,x]) - (o[c+1,y,x] - o[c,y,x]), Dx Dc likewise along x,
// every sum over the indices whose operands all lie inside the image: nothing is padded and nothing of a
// frame around the image is used.  phi'(d) = d / sqrt(d^2 + eps^2); eps = 0: sign(d), sign(0) = 0 (torch's
// abs backward).  Part of dipnet.hip's translation unit.
//
// One gathering pass: a thread owns 4 consecutive elements of a row and sums, per element, the derivative
// terms of the differences it takes part in (up to 4 spatial, 2 band, 8 SSTV) in a fixed order, then adds
// the result to gout -- no float atomics on the gradient, reruns are bit-identical.  A difference shared
// by several elements is recomputed by each from the same operands in the same association, so every copy
// has the same bits and gout is the exact gradient of the fp32 function evaluated.  The value counts each
// difference once, at its lowest-index element, in fp64 per thread; one fp64 atomicAdd per workgroup into
// loss_acc, as k_masked_mse adds its own sum.
//
// Memory path (MI355X_MICROARCH.md, memory hierarchy): the thread reads the 15-point stencil of its 4
// elements as 3 planes x (6 + 4 + 4) floats = 10.5 loads per element.  The 14 loads of one plane are the
// row segments its neighbour threads and the workgroups one row away read too: L1 / L2 hits.  The planes
// c - 1 and c + 1 are Hf Wf floats away and are the centre planes of workgroups that run at the same time
// on other XCDs, so a line reaches up to three L2s, the extra two fills from the Infinity Cache (the
// output was written by the last conv a few kernels earlier: 30 MB at 198 x 196 x 196).  An LDS tile would
// not lower that: the L2-level request volume, 10.5 x 4 B x 7.6 M = 320 MB, takes ~9 us at the L2's
// 34.5 TB/s, below the ~15 us of the compulsory 91 MB (out read once, gout read and written) at the
// 6.3 TB/s HBM rate, and staging a 3-plane tile with its cross halo through ds_write (38-51 TB/s
// aggregate) costs as much as the L2 reads it replaces, plus a barrier.  So: plain loads, L2 reuse, no LDS.
#pragma once
#include "dip_launch.h"

namespace lrs {

struct TvArgs {
    const float *out;      // the image's element (0, 0, 0) inside the frame
    float *gout;           // the same element of the gradient buffer (nullable)
    double *loss_acc;      // nullable
    int C, H, W, Wf;       // the image; the frame's row stride
    int64_t plane;         // Hf Wf
    float gsp, gbd, gss;   // w / N: the gradient's weights
    float wsp, wbd, wss;   // w: the value's (loss_acc holds N R, as it holds the squared-error sum)
    float eps2;
    unsigned S, items;     // 4-element strips per row; C H S
};

// phi'(d), and phi(d) into ph
__device__ __forceinline__ float tv_dphi(float d, float eps2, float &ph) {
    if (eps2 == 0.0f) {   // (eps so small that its square is 0 in fp32 takes this branch too)
        ph = fabsf(d);
        return (float)(d > 0.0f) - (float)(d < 0.0f);
    }
    const float s = d * d + eps2, r = rsqrtf(s);
    ph = s * r;
    return d * r;
}

// v[0..4) = row[x0 .. x0 + 4), columns at or beyond W read as 0.  kVec: one 16-byte load (the caller
// guarantees alignment and that the segment ends inside the frame's row); else the columns inside only.
template <bool kVec>
__device__ __forceinline__ void tv_load4(const float *__restrict__ row, int x0, int W, float *v) {
    if (kVec) {
        const float4 q = *reinterpret_cast<const float4 *>(row + x0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
#pragma unroll
        for (int j = 1; j < 4; ++j) v[j] = x0 + j < W ? v[j] : 0.0f;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = x0 + j < W ? row[x0 + j] : 0.0f;
    }
}

// grid-stride over the C H S strips, 256 threads.  kVec: out, gout 16-byte aligned at every strip (the
// launcher checks the bases, Wf % 4 and left % 4); both forms run the same arithmetic on the same
// registers and differ in the loads and stores only: the same bits.
template <bool kVec>
__global__ __launch_bounds__(256) void k_sstv(const TvArgs a) {
    __shared__ double red[8];
    const bool planes = a.wbd != 0.0f || a.wss != 0.0f, corners = a.wss != 0.0f;
    double vs = 0.0, vb = 0.0, vq = 0.0;   // the value's three sums
    for (unsigned it = blockIdx.x * 256u + threadIdx.x; it < a.items; it += gridDim.x * 256u) {
        const unsigned s = it % a.S, r = it / a.S;
        const int y = (int)(r % (unsigned)a.H), c = (int)(r / (unsigned)a.H), x0 = 4 * (int)s;
        const int64_t at = (int64_t)c * a.plane + (int64_t)y * a.Wf;
        const bool vup = y > 0, vdn = y + 1 < a.H, vc[3] = {c > 0, true, c + 1 < a.C};
        // planes c - 1, c, c + 1: the row's columns x0 - 1 .. x0 + 4 and the rows above and below
        float ctr[3][6], up[3][4], dn[3][4];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int k = 0; k < 6; ++k) ctr[p][k] = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) up[p][k] = dn[p][k] = 0.0f;
            if (!vc[p] || (p != 1 && !planes)) continue;
            const float *row = a.out + at + (int64_t)(p - 1) * a.plane;
            tv_load4<kVec>(row, x0, a.W, &ctr[p][1]);
            if (x0 > 0) ctr[p][0] = row[x0 - 1];
            if (x0 + 4 < a.W) ctr[p][5] = row[x0 + 4];
            if (!(corners || (p == 1 && a.wsp != 0.0f))) continue;
            if (vup) tv_load4<kVec>(row - a.Wf, x0, a.W, up[p]);
            if (vdn) tv_load4<kVec>(row + a.Wf, x0, a.W, dn[p]);
        }
        float g[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = j + 1, x = x0 + j;
            const bool vl = x > 0, vr = x + 1 < a.W, in = x < a.W;
            const float o = ctr[1][k];
            float gs = 0.0f, gb = 0.0f, gq = 0.0f, ph;
            if (a.wsp != 0.0f) {
                if (vdn) { gs -= tv_dphi(dn[1][j] - o, a.eps2, ph); if (in) vs += (double)ph; }
                if (vup) gs += tv_dphi(o - up[1][j], a.eps2, ph);
                if (vr) { gs -= tv_dphi(ctr[1][k + 1] - o, a.eps2, ph); vs += (double)ph; }
                if (vl) gs += tv_dphi(o - ctr[1][k - 1], a.eps2, ph);
            }
            if (a.wbd != 0.0f) {
                if (vc[2]) { gb -= tv_dphi(ctr[2][k] - o, a.eps2, ph); if (in) vb += (double)ph; }
                if (vc[0]) gb += tv_dphi(o - ctr[0][k], a.eps2, ph);
            }
            if (corners) {
                // the band pair (lo, hi) = (c - 1, c), then (c, c + 1); the element is the difference's
                // high band in the first (coefficient + with the high row / column) and its low band in
                // the second (coefficient - there); the pair (c, c + 1) at (y, x) is the one it owns
#pragma unroll
                for (int lo = 0; lo < 2; ++lo) {
                    if (!vc[2 * lo]) continue;
                    const int hi = lo + 1;
                    const float sg = lo == 0 ? 1.0f : -1.0f, dc = ctr[hi][k] - ctr[lo][k];
                    if (vup) gq += sg * tv_dphi(dc - (up[hi][j] - up[lo][j]), a.eps2, ph);
                    if (vdn) {
                        gq -= sg * tv_dphi((dn[hi][j] - dn[lo][j]) - dc, a.eps2, ph);
                        if (lo == 1 && in) vq += (double)ph;
                    }
                    if (vl) gq += sg * tv_dphi(dc - (ctr[hi][k - 1] - ctr[lo][k - 1]), a.eps2, ph);
                    if (vr) {
                        gq -= sg * tv_dphi((ctr[hi][k + 1] - ctr[lo][k + 1]) - dc, a.eps2, ph);
                        if (lo == 1) vq += (double)ph;
                    }
                }
            }
            g[j] = (a.gsp * gs + a.gbd * gb) + a.gss * gq;
        }
        if (!a.gout) continue;
        float *gp = a.gout + at + x0;
        if (kVec && x0 + 4 <= a.W) {
            float4 q = *reinterpret_cast<float4 *>(gp);
            q.x += g[0]; q.y += g[1]; q.z += g[2]; q.w += g[3];
            *reinterpret_cast<float4 *>(gp) = q;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < a.W) gp[j] += g[j];
        }
    }
    if (!a.loss_acc) return;
    const double v = block_sum_d((double)a.wsp * vs + (double)a.wbd * vb + (double)a.wss * vq, red);
    if (threadIdx.x == 0) atomicAdd(a.loss_acc, v);
}

}  // namespace lrs

namespace {   // (internal linkage: this header is part of dipnet.hip's translation unit only)

// R of the H x W image at (top, left) of out[C][Hf][Wf]: gout (nullable) += dR/do on the image, loss_acc
// (nullable) += N R.  All three weights 0: nothing is launched.
int sstv(const float *out, int C, int Hf, int Wf, int top, int left, int H, int W, float w_sp, float w_bd,
         float w_ss, float eps, int64_t n_mean, float *gout, double *loss_acc, hipStream_t st) {
    if (!out || C <= 0 || Hf <= 0 || Wf <= 0 || H <= 0 || W <= 0 || top < 0 || left < 0 || top > Hf - H ||
        left > Wf - W || !(w_sp >= 0.0f) || !(w_bd >= 0.0f) || !(w_ss >= 0.0f) || !(eps >= 0.0f) || n_mean <= 0)
        return LRS_E_INVALID;
    if ((w_sp == 0.0f && w_bd == 0.0f && w_ss == 0.0f) || (!gout && !loss_acc)) return LRS_OK;
    const int64_t S = (W + 3) / 4, items = (int64_t)C * H * S;
    if (items > INT32_MAX) return LRS_E_UNSUPPORTED;
    const int64_t base = (int64_t)top * Wf + left;
    lrs::TvArgs a{out + base, gout ? gout + base : nullptr, loss_acc, C, H, W, Wf, (int64_t)Hf * Wf,
                  (float)((double)w_sp / (double)n_mean), (float)((double)w_bd / (double)n_mean),
                  (float)((double)w_ss / (double)n_mean), w_sp, w_bd, w_ss, eps * eps, (unsigned)S, (unsigned)items};
    // ~2048 workgroups at most (grid-stride beyond): enough waves for every CU, few loss atomics
    const unsigned grid = (unsigned)std::min<int64_t>((items + 255) / 256, 2048);
    const bool vec = Wf % 4 == 0 && left % 4 == 0 && al16(out) && (!gout || al16(gout));
    if (vec) hipLaunchKernelGGL(lrs::k_sstv<true>, dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(lrs::k_sstv<false>, dim3(grid), dim3(256), 0, st, a);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

}  // namespace

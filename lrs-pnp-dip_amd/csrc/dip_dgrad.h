// The kernels that finish a DIP conv's data gradient after its GEMM: the reflection-border corrections
// of the effective-kernel form and the fold of the padded-domain form (dip_launch.h conv_dgrad).
#pragma once

#include "dip_kernels.h"   // padded_sources

namespace lrs {

// Reflection-pad corrections of the effective-kernel data gradient of an upsampled, reflection-
// padded 3 x 3 conv (pad 1).  The stride-2 4 x 4 conv over dL/dz treats the padded border as zeros;
// the reference's ReflectionPad2d(1) also feeds padded row -1 from row 1 and row Hu from Hu - 2
// (same for columns): extra (oy, ky) pairs (0, 0) -> source row 0 and (Hu - 1, 2) -> row Hs - 1,
// and likewise (ox, kx) for the columns.  Four "lines": 0 / 1 = source rows 0 / Hs - 1 take every
// term with a reflected row (any column, reflected or not); 2 / 3 = source columns 0 / Ws - 1 every
// term with a reflected column and an unreflected row, so each term is counted once.  Three wide
// launches (k_up_border_s, _mm, _add), scratch in the conv's col-gradient buffer:
//   S[line][co][j][pos]  = the line's dL/dz summed over the positions that map to source pos via
//                          tap j (j = kx for rows, ky for columns)
//   corr[line][c][pos]   = sum_{co, j} W[co][c][tap(line, j)] S[line][co][j][pos]
// then gx[c][perimeter pixel] += its row-line and column-line corrections.  w = the conv's fp32
// weights (W / sigma) [Cout][Cin][3][3].
constexpr int kUbC = 4, kUbCo = 32;

__device__ __forceinline__ int ub_len(int line, int Hs, int Ws) { return line < 2 ? Ws : Hs; }

__global__ __launch_bounds__(256) void k_up_border_s(const float *__restrict__ gz, int Cout, int Hs, int Ws, int Lmax,
                                                     float *__restrict__ S) {
    const int co = blockIdx.y, e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 4 * 3 * Lmax) return;
    const int line = e / (3 * Lmax), j = (e / Lmax) % 3, pos = e % Lmax;
    const int Hu = 2 * Hs, Wu = 2 * Ws, rows = line < 2, L = ub_len(line, Hs, Ws), Lu = rows ? Wu : Hu;
    float v = 0.0f;
    if (pos < L) {
        const int ofix = (line & 1) == 0 ? 0 : (rows ? Hu - 1 : Wu - 1);
        const float *g = gz + (int64_t)co * Hu * Wu;
        for (int o = max(0, 2 * pos - 2); o <= min(Lu - 1, 2 * pos + 3); ++o) {
            int u = o + j - 1;
            if (rows) u = u < 0 ? -u : (u >= Lu ? 2 * (Lu - 1) - u : u);   // along x: reflected ends included
            else if (u < 0 || u >= Lu) continue;                          // along y: unreflected rows only
            if ((u >> 1) == pos) v += g[rows ? (int64_t)ofix * Wu + o : (int64_t)o * Wu + ofix];
        }
    }
    S[(((int64_t)line * Cout + co) * 3 + j) * Lmax + pos] = v;
}

__global__ __launch_bounds__(256) void k_up_border_mm(const float *__restrict__ S, const float *__restrict__ w, int Cin,
                                                      int Cout, int Hs, int Ws, int Lmax, float *__restrict__ corr) {
    __shared__ float Ss[kUbCo * 3 * 128], Wl[kUbCo * kUbC * 3];
    const int line = blockIdx.x, c0 = blockIdx.y * kUbC, p0 = blockIdx.z * 128;
    const int rows = line < 2, L = ub_len(line, Hs, Ws), tfix = (line & 1) == 0 ? 0 : 2;
    const int cl = threadIdx.x >> 7, pl = threadIdx.x & 127;   // 2 channels x 128 positions per pass
    float acc[2] = {0.0f, 0.0f};
    for (int co0 = 0; co0 < Cout; co0 += kUbCo) {
        __syncthreads();
        float sv[kUbCo * 3 * 128 / 256];   // all 48 loads issued before any LDS store (clamped, then masked)
#pragma unroll
        for (int u = 0; u < kUbCo * 3 * 128 / 256; ++u) {
            const int e = threadIdx.x + 256 * u;
            const int col = e / 384, j = (e >> 7) % 3, pos = p0 + (e & 127), co = co0 + col;
            const int cc = min(co, Cout - 1), pp = min(pos, Lmax - 1);
            sv[u] = S[(((int64_t)line * Cout + cc) * 3 + j) * Lmax + pp];
        }
#pragma unroll
        for (int u = 0; u < kUbCo * 3 * 128 / 256; ++u) {
            const int e = threadIdx.x + 256 * u;
            const int col = e / 384, pos = p0 + (e & 127), co = co0 + col;
            Ss[e] = (co < Cout && pos < L) ? sv[u] : 0.0f;
        }
        for (int e = threadIdx.x; e < kUbCo * kUbC * 3; e += blockDim.x) {
            const int col = e / (kUbC * 3), c = c0 + (e / 3) % kUbC, j = e % 3, co = co0 + col;
            Wl[e] = (co < Cout && c < Cin) ? w[((int64_t)co * Cin + c) * 9 + (rows ? tfix * 3 + j : j * 3 + tfix)] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = 2 * h + cl;
            float a = acc[h];
            for (int col = 0; col < kUbCo; ++col)
#pragma unroll
                for (int j = 0; j < 3; ++j) a = __fmaf_rn(Wl[(col * kUbC + c) * 3 + j], Ss[(col * 3 + j) * 128 + pl], a);
            acc[h] = a;
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int c = c0 + 2 * h + cl, pos = p0 + pl;
        if (c < Cin && pos < L) corr[((int64_t)line * Cin + c) * Lmax + pos] = acc[h];
    }
}

__global__ __launch_bounds__(256) void k_up_border_add(const float *__restrict__ corr, int Cin, int Hs, int Ws,
                                                       int Lmax, float *__restrict__ gx) {
    const int nper = 2 * Ws + 2 * (Hs - 2);
    const int idx = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
    if (idx >= nper) return;
    int sy, sx;
    if (idx < Ws) { sy = 0; sx = idx; }
    else if (idx < 2 * Ws) { sy = Hs - 1; sx = idx - Ws; }
    else { const int r = idx - 2 * Ws; sy = 1 + (r >> 1); sx = (r & 1) ? Ws - 1 : 0; }
    float v = 0.0f;
    if (sy == 0) v += corr[((int64_t)0 * Cin + c) * Lmax + sx];
    if (sy == Hs - 1) v += corr[((int64_t)1 * Cin + c) * Lmax + sx];
    if (sx == 0) v += corr[((int64_t)2 * Cin + c) * Lmax + sy];
    if (sx == Ws - 1) v += corr[((int64_t)3 * Cin + c) * Lmax + sy];
    float *o = gx + ((int64_t)c * Hs + sy) * Ws + sx;
    *o = *o + v;
}

// gx[c][sy][sx] (+)= sum over the x2 upsample children u of sum over the padded positions that
// read u (direct + reflection mirrors, padded_sources) of gxp[c][iy][ix], where gxp is the sum of
// nsplit split-K partials (stride zstride floats; the data-gradient GEMM's split-K finished here, in
// k_gemm_reduce's order per position)
__device__ __forceinline__ float fold_term(const float *__restrict__ src, int nsplit, int64_t zstride, int64_t i) {
    if (nsplit == 1) return src[i];
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int z0 = 0; z0 < nsplit; z0 += 8) {
        float p[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) p[e] = z0 + e < nsplit ? src[(int64_t)(z0 + e) * zstride + i] : 0.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (z0 + e < nsplit) acc[e] += p[e];
    }
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
}

__global__ __launch_bounds__(256) void k_fold_pad(const float *__restrict__ gxp, int nsplit, int64_t zstride,
                                                  ConvGeom gm, float *__restrict__ gx, int accum) {
    const int HW = gm.Hs * gm.Ws, Wp = gm.Wu + 2 * gm.pad, Qp = (gm.Hu + 2 * gm.pad) * Wp;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= HW) return;
    const int sy = q / gm.Ws, sx = q - sy * gm.Ws;
    const int nup = gm.up ? 2 : 1;
    for (int c = blockIdx.y; c < gm.Cin; c += gridDim.y) {
        const float *src = gxp + (int64_t)c * Qp;
        float acc = 0.0f;
        for (int a = 0; a < nup; ++a) {
            int iys[3];
            const int ny = padded_sources(gm.up ? 2 * sy + a : sy, gm.Hu, gm.pad, gm.pad_mode, iys);
            for (int b = 0; b < nup; ++b) {
                int ixs[3];
                const int nx = padded_sources(gm.up ? 2 * sx + b : sx, gm.Wu, gm.pad, gm.pad_mode, ixs);
                for (int py = 0; py < ny; ++py)
                    for (int px = 0; px < nx; ++px) acc += fold_term(src, nsplit, zstride, iys[py] * Wp + ixs[px]);
            }
        }
        const int64_t i = (int64_t)c * HW + q;
        gx[i] = accum ? gx[i] + acc : acc;
    }
}

// k_fold_pad for one partial (nsplit == 1, no upsample; a data-gradient GEMM with enough tiles, e.g.
// the 512^2 layers of configs[3]): grid (row quads, Cin), a thread = 4 consecutive source x of one
// row, float4 stores (Ws % 4 == 0).  Per pixel the same padded sources in the same order as
// k_fold_pad, so the result is bit-identical.
__global__ __launch_bounds__(256) void k_fold_pad1q(const float *__restrict__ gxp, ConvGeom gm, float *__restrict__ gx,
                                                    int accum) {
    const int W4 = gm.Ws >> 2, Wp = gm.Wu + 2 * gm.pad, Qp = (gm.Hu + 2 * gm.pad) * Wp;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= gm.Hs * W4) return;
    const int c = blockIdx.y, sy = t / W4, sx0 = 4 * (t - sy * W4);
    const float *src = gxp + (int64_t)c * Qp;
    int iys[3];
    const int ny = padded_sources(sy, gm.Hu, gm.pad, gm.pad_mode, iys);
    float acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int ixs[3];
        const int nx = padded_sources(sx0 + e, gm.Wu, gm.pad, gm.pad_mode, ixs);
        float a = 0.0f;
        for (int py = 0; py < ny; ++py)
            for (int px = 0; px < nx; ++px) a += src[iys[py] * Wp + ixs[px]];
        acc[e] = a;
    }
    float4 *o = reinterpret_cast<float4 *>(gx + ((int64_t)c * gm.Hs + sy) * gm.Ws + sx0);
    float4 r = make_float4(acc[0], acc[1], acc[2], acc[3]);
    if (accum) {
        const float4 p = *o;
        r = make_float4(p.x + r.x, p.y + r.y, p.z + r.z, p.w + r.w);
    }
    *o = r;
}

}  // namespace lrs

// On-device quality monitor: MPSNR / SAM / relative error of X against the clean cube in one
// pass over both, optionally restricted to a region (the hole), and a device-side "keep if better" snapshot.
//
// lrs_cube_quality_f32, three stream-ordered launches, every sum in a fixed order (no float atomics):
//   k_quality_partial : workgroup s owns a slab of pixel rows, its waves take the slab's rows in turn.  A
//                       row (one pixel's spectrum) is contiguous, so lane l reads bands l, l + 64, ...: the
//                       per-band sums (sse, n, c^2 over the region) stay in that lane's registers across
//                       rows, and the pixel's <x,x>, <c,c>, <x,c> are three wave sums.  The wave sums are
//                       uniform; lane (row mod 64) keeps them, and every 64 rows each lane forms its own
//                       pixel's angle, so the sqrt / divide / acos run once per 64 rows.  The waves' band
//                       sums meet in LDS in wave order; the slab's partials go to ws.
//   k_quality_bands   : per band, the slabs in fixed order (8 slab groups per band, then the groups in
//                       order): sse_b, n_b, c2_b and psnr_b.
//   k_quality_final   : one wave: the bands and the slabs' angle sums in fixed order -> q[0..3].
// Above kQRegBands bands the per-band sums no longer fit the registers: the same kernel body, one wave per
// workgroup, keeps them in its slab's row of ws instead (read-modify-write by the lane that owns the band).
// X, C and region are read once in either form.
#include <math.h>

#include "lrs_common.h"

namespace lrs {

constexpr int kQSlabs = 512;       // at most this many slabs (workgroups of the first pass)
constexpr int kQWaves = 8;         // waves of a workgroup, register form
constexpr int kQRegBands = 512;    // widest cube of the register form (8 chunks of 64 bands per lane)
constexpr int kQBandTile = 32;     // bands per workgroup of k_quality_bands
constexpr int kQBandGroups = 8;    // slab groups per band there

struct QPix {
    double xx, cc, xc;
    int any;
};

// one entry: the region's sums of its band (sse, n, c2) and the pixel's spectrum sums
__device__ __forceinline__ void q_entry(float xf, float cf, int r, double &sse, double &cnt, double &c2, QPix &s) {
    const double x = (double)xf, c = (double)cf;
    if (r) {
        const double d = x - c;
        sse = __fma_rn(d, d, sse);
        c2 = __fma_rn(c, c, c2);
        cnt += 1.0;
    }
    s.xx = __fma_rn(x, x, s.xx);
    s.cc = __fma_rn(c, c, s.cc);
    s.xc = __fma_rn(x, c, s.xc);
    s.any |= r;
}

// the angle of the pixel this lane holds, added to the lane's sums (a zero-norm spectrum is not counted)
__device__ __forceinline__ void q_angle(int &held, double xx, double cc, double xc, double &ang, double &npix) {
    if (held) {
        const double den = sqrt(xx) * sqrt(cc);
        if (den > 0.0) {
            const double cs = fmin(1.0, fmax(-1.0, xc / den));
            ang += acos(cs);
            npix += 1.0;
        }
    }
    held = 0;
}

// part: [nslab][3][B] (sse, n, c2), sam: [nslab][2] (sum of angles, pixels).  NCH > 0: NCH chunks of 64 bands
// in registers, kQWaves waves; NCH == 0: any B, one wave, the band sums in the slab's row of part.
template <int NCH>
__global__ __launch_bounds__(NCH ? kQWaves * 64 : 64) void k_quality_partial(
    const float *__restrict__ X, const float *__restrict__ C, const uint8_t *__restrict__ region, int64_t P, int B,
    int64_t rows, double *part, double *__restrict__ sam) {
    constexpr int NW = NCH ? kQWaves : 1, NR = NCH ? NCH : 1;
    __shared__ double sh[NW][NR * 64];
    __shared__ double sh_sam[NW][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * rows, r1 = min<int64_t>(P, r0 + rows);
    double *mine = part + (int64_t)blockIdx.x * 3 * B;
    double acc[3][NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) acc[0][k] = acc[1][k] = acc[2][k] = 0.0;
    if (NCH == 0)
        for (int b = lane; b < B; b += 64) mine[b] = mine[B + b] = mine[2 * B + b] = 0.0;
    double hxx = 0.0, hcc = 0.0, hxc = 0.0, ang = 0.0, npix = 0.0;
    int held = 0, turn = 0;
    for (int64_t p = r0 + w; p < r1; p += NW, ++turn) {
        const float *x = X + p * B, *c = C + p * B;
        const uint8_t *rg = region ? region + p * B : nullptr;
        QPix s = {0.0, 0.0, 0.0, 0};
        if (NCH) {
#pragma unroll
            for (int k = 0; k < NR; ++k) {
                const int b = k * 64 + lane;
                if (b < B) q_entry(x[b], c[b], rg ? rg[b] == 1 : 1, acc[0][k], acc[1][k], acc[2][k], s);
            }
        } else {
            for (int b = lane; b < B; b += 64) {
                double sse = mine[b], cnt = mine[B + b], c2 = mine[2 * B + b];
                q_entry(x[b], c[b], rg ? rg[b] == 1 : 1, sse, cnt, c2, s);
                mine[b] = sse, mine[B + b] = cnt, mine[2 * B + b] = c2;
            }
        }
        const double sxx = wave_sum_butterfly(s.xx), scc = wave_sum_butterfly(s.cc), sxc = wave_sum_butterfly(s.xc);
        const int counted = __ballot(s.any) != 0;
        if (lane == (turn & 63)) hxx = sxx, hcc = scc, hxc = sxc, held = counted;
        if ((turn & 63) == 63) q_angle(held, hxx, hcc, hxc, ang, npix);
    }
    q_angle(held, hxx, hcc, hxc, ang, npix);
    ang = wave_sum_butterfly(ang);
    npix = wave_sum_butterfly(npix);
    if (NCH == 0) {
        if (lane == 0) sam[2 * blockIdx.x] = ang, sam[2 * blockIdx.x + 1] = npix;
        return;
    }
    if (lane == 0) sh_sam[w][0] = ang, sh_sam[w][1] = npix;
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int k = 0; k < NR; ++k) sh[w][k * 64 + lane] = acc[a][k];
        __syncthreads();
        for (int b = threadIdx.x; b < B; b += NW * 64) {
            double t = sh[0][b];
            for (int v = 1; v < NW; ++v) t += sh[v][b];
            mine[a * B + b] = t;
        }
        __syncthreads();
    }
    if (threadIdx.x < 2) {
        double t = sh_sam[0][threadIdx.x];
        for (int v = 1; v < NW; ++v) t += sh_sam[v][threadIdx.x];
        sam[2 * blockIdx.x + threadIdx.x] = t;
    }
}

// band: [4][B] (psnr_b, sse_b, n_b, c2_b)
__global__ __launch_bounds__(kQBandTile *kQBandGroups) void k_quality_bands(const double *__restrict__ part, int nslab,
                                                                            int B, double *__restrict__ band,
                                                                            double *__restrict__ psnr_bands) {
    __shared__ double sh[3][kQBandGroups][kQBandTile];
    const int j = threadIdx.x % kQBandTile, g = threadIdx.x / kQBandTile, b = blockIdx.x * kQBandTile + j;
    const int per = (nslab + kQBandGroups - 1) / kQBandGroups, k0 = g * per, k1 = min(nslab, k0 + per);
    double s[3] = {0.0, 0.0, 0.0};
    if (b < B)
        for (int k = k0; k < k1; ++k) {
            const double *row = part + (int64_t)k * 3 * B + b;
            s[0] += row[0], s[1] += row[B], s[2] += row[2 * B];
        }
    for (int a = 0; a < 3; ++a) sh[a][g][j] = s[a];
    __syncthreads();
    if (g || b >= B) return;
    for (int a = 0; a < 3; ++a) {
        s[a] = sh[a][0][j];
        for (int v = 1; v < kQBandGroups; ++v) s[a] += sh[a][v][j];
    }
    double psnr = nan("");
    if (s[1] > 0.0) {
        const double mse = s[0] / s[1];
        psnr = mse < 1.0e-10 ? 100.0 : 10.0 * log10(255.0 / sqrt(mse));
    }
    band[b] = psnr, band[B + b] = s[0], band[2 * B + b] = s[1], band[3 * B + b] = s[2];
    if (psnr_bands) psnr_bands[b] = psnr;
}

__global__ __launch_bounds__(64) void k_quality_final(const double *__restrict__ band, const double *__restrict__ sam,
                                                      int nslab, int B, double *__restrict__ q) {
    const int lane = threadIdx.x;
    double ps = 0.0, nb = 0.0, sse = 0.0, c2 = 0.0, ang = 0.0, npix = 0.0;
    for (int b = lane; b < B; b += 64) {
        if (band[2 * B + b] > 0.0) ps += band[b], nb += 1.0;
        sse += band[B + b];
        c2 += band[3 * B + b];
    }
    for (int k = lane; k < nslab; k += 64) ang += sam[2 * k], npix += sam[2 * k + 1];
    ps = wave_sum_butterfly(ps), nb = wave_sum_butterfly(nb), sse = wave_sum_butterfly(sse);
    c2 = wave_sum_butterfly(c2), ang = wave_sum_butterfly(ang), npix = wave_sum_butterfly(npix);
    if (lane) return;
    q[0] = nb > 0.0 ? ps / nb : nan("");
    q[1] = npix > 0.0 ? ang / npix * (180.0 / 3.14159265358979323846) : nan("");
    q[2] = c2 > 0.0 ? sqrt(sse) / sqrt(c2) : nan("");
    q[3] = npix;
}

// ---- keep if better ------------------------------------------------------------------------------------
__device__ __forceinline__ bool q_better(double s, double b, int sign) {
    return s == s && (b != b || (double)sign * s > (double)sign * b);
}

// every thread reads the same two doubles and decides alike; best is written by k_keep_update, the next launch
__global__ __launch_bounds__(256) void k_keep_copy(const double *__restrict__ score, const double *__restrict__ best,
                                                   int sign, const float *__restrict__ src, float *__restrict__ dst,
                                                   int64_t n, int vec) {
    if (!q_better(score[0], best[0], sign)) return;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, nt = (int64_t)gridDim.x * 256;
    int64_t done = 0;
    if (vec) {
        const int64_t n4 = n >> 2;
        const float4 *s4 = (const float4 *)src;
        float4 *d4 = (float4 *)dst;
        for (int64_t i = t; i < n4; i += nt) d4[i] = s4[i];
        done = n4 << 2;
    }
    for (int64_t i = done + t; i < n; i += nt) dst[i] = src[i];
}

__global__ void k_keep_update(const double *__restrict__ score, int sign, int iteration, double *best) {
    const double s = score[0];
    if (q_better(s, best[0], sign)) best[0] = s, best[1] = (double)iteration;
}

static int64_t q_rows(int64_t P, int64_t B) {
    const int64_t rows = (P + kQSlabs - 1) / kQSlabs;
    return B <= kQRegBands && rows < kQWaves ? kQWaves : rows;   // register form: a row per wave at the least
}

}  // namespace lrs

using namespace lrs;

extern "C" size_t lrs_cube_quality_workspace(int64_t P, int64_t B) {
    if (P <= 0 || B <= 0 || P >= ((int64_t)1 << 31) / B + (((int64_t)1 << 31) % B != 0)) return 0;
    return ((size_t)kQSlabs * (3 * (size_t)B + 2) + 4 * (size_t)B) * sizeof(double);
}

extern "C" int lrs_cube_quality_f32(const float *X, const float *C, const uint8_t *region, int64_t P, int64_t B,
                                    double *q, double *psnr_bands, void *ws, size_t ws_bytes, void *stream) {
    if (!X || !C || !q || !ws || P <= 0 || B <= 0) return LRS_E_INVALID;
    const size_t need = lrs_cube_quality_workspace(P, B);
    if (need == 0) return LRS_E_UNSUPPORTED;   // P B >= 2^31
    if (ws_bytes < need) return LRS_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int64_t rows = q_rows(P, B);
    const int nslab = (int)((P + rows - 1) / rows), Bi = (int)B;
    double *part = (double *)ws, *sam = part + (size_t)kQSlabs * 3 * B, *band = sam + 2 * kQSlabs;
    const dim3 grid((unsigned)nslab);
#define LRS_Q_PARTIAL(NCH, NT) \
    hipLaunchKernelGGL(k_quality_partial<NCH>, grid, dim3(NT), 0, st, X, C, region, P, Bi, rows, part, sam)
    if (B <= 64)
        LRS_Q_PARTIAL(1, kQWaves * 64);
    else if (B <= 128)
        LRS_Q_PARTIAL(2, kQWaves * 64);
    else if (B <= 256)
        LRS_Q_PARTIAL(4, kQWaves * 64);
    else if (B <= kQRegBands)
        LRS_Q_PARTIAL(8, kQWaves * 64);
    else
        LRS_Q_PARTIAL(0, 64);
#undef LRS_Q_PARTIAL
    LRS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_quality_bands, dim3((unsigned)((B + kQBandTile - 1) / kQBandTile)),
                       dim3(kQBandTile * kQBandGroups), 0, st, (const double *)part, nslab, Bi, band, psnr_bands);
    LRS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_quality_final, dim3(1), dim3(64), 0, st, (const double *)band, (const double *)sam, nslab, Bi,
                       q);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

extern "C" int lrs_keep_best_f32(const double *score, int sign, int32_t iteration, const float *src, float *dst,
                                 int64_t n, double *best, void *stream) {
    if (!score || !src || !dst || !best || n <= 0 || (sign != 1 && sign != -1)) return LRS_E_INVALID;
    const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst, len = (uintptr_t)n * sizeof(float);
    if (s0 < d0 + len && d0 < s0 + len) return LRS_E_INVALID;   // src may not alias dst
    hipStream_t st = (hipStream_t)stream;
    const int vec = ((s0 | d0) & 15) == 0;
    int64_t blocks = (n + 1023) / 1024;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_keep_copy, dim3((unsigned)blocks), dim3(256), 0, st, score, (const double *)best, sign, src,
                       dst, n, vec);
    LRS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_keep_update, dim3(1), dim3(1), 0, st, score, sign, (int)iteration, best);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

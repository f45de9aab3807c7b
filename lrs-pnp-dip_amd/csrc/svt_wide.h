// The wide-band SVT path, 256 < B <= 512: its constants and its Gram kernel (the shape table in
// svt_ws.h and the launchers in svt.hip hold the dispatch).
// The one-workgroup kernels of B <= 256 keep every 16 x 16 tile pair of the Gram, and every column
// of 16 rows of U, in one workgroup's registers; here both products are tiled over a 2-D grid so
// that a workgroup's accumulators stay below those kernels' however wide the cube is.
#pragma once

#include "lrs_common.h"

namespace lrs {

constexpr int kWideMaxBp = 512;

// The apply of wide cubes (k_svt_apply_f<kWideApRows, kWideApTiles, 0>, svt_apply.h): a wave owns
// 16 RT rows and 16 NTL columns and walks K = B in ceil(B / 8) pairs of k-steps of 4, so Fp holds
// 2 ceil(B / 8) k-steps.
__host__ __device__ constexpr int wide_ap_steps(int64_t B) { return 2 * (int)((B + 7) / 8); }
constexpr int kWideApRows = 2;    // RT: 32 rows per wave, 128 per workgroup
constexpr int kWideApTiles = 8;   // NTL: 128 columns per workgroup (16 accumulator tiles per wave)

// ---- 1w. Gram G = Z^T Z on the fp64 matrix cores, row slab x column-panel pair ----------------
// Panels of 64 columns (4 tiles of 16): workgroup (slab, pair (pa <= pb)) stages the slab's rows of
// both panels kWideChunk at a time into LDS (Z = X + c2*L2 formed on the way, the float32 expression
// of k_gram_mfma and the apply kernels), and wave w accumulates the 4 tiles (4 pa + w, 4 pb + b),
// b = 0..3: 4 accumulators per wave.  Fragments as in k_gram_mfma: per k-step of 4 rows a lane
// reads Z[r + (l>>4)][16 t + (l&15)].  Tiles (a <= b) go to partial[slab][pair index of (a, b) among
// the nt (nt + 1) / 2 upper tile pairs][16*16], the layout k_gram_reduce16 sums in fixed order; the
// tiles below the diagonal of a pair (pa, pa) and those past nt are computed and dropped.
constexpr int kWideSlabs = 32;
constexpr int kWidePanel = 64;
constexpr int kWideChunk = 32;                    // rows per LDS chunk
constexpr int kWideLd = 2 * kWidePanel + 16;      // row stride: lane groups 16 banks apart

__host__ __device__ constexpr int wide_npanels(int B) { return (B + kWidePanel - 1) / kWidePanel; }

__global__ __launch_bounds__(256) void k_gram_wide(const float *__restrict__ X, const float *__restrict__ L2,
                                                   float c2, int64_t P, int B, int64_t rows_per_slab, int nt,
                                                   double *__restrict__ partial) {
    typedef double doublex4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) float Zs[kWideChunk * kWideLd];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, jl = lane & 15;
    const int npan = wide_npanels(B);
    int pa = 0, rem = blockIdx.y;
    while (rem >= npan - pa) {
        rem -= npan - pa;
        ++pa;
    }
    const int pb = pa + rem;
    const bool diag = pa == pb;
    const int64_t pbeg = (int64_t)blockIdx.x * rows_per_slab, pend = min<int64_t>(P, pbeg + rows_per_slab);
    // staging: thread -> LDS column cl (0..63 panel pa, 64..127 panel pb), rows (tid >> 7) + 2u
    const int cl = tid & 127, hp = cl >> 6;
    const int gc = kWidePanel * (hp ? pb : pa) + (cl & 63);
    const bool cok = gc < B && !(hp && diag);
    const int boff = diag ? 0 : kWidePanel;
    doublex4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = doublex4{0.0, 0.0, 0.0, 0.0};
    for (int64_t c0 = pbeg; c0 < pend; c0 += kWideChunk) {
        const int rows = (int)min<int64_t>(kWideChunk, pend - c0);
        float z[kWideChunk / 2];
#pragma unroll
        for (int u = 0; u < kWideChunk / 2; ++u) {
            const int r = (tid >> 7) + 2 * u;
            z[u] = 0.f;
            if (cok && r < rows) {
                const int64_t o = (c0 + r) * B + gc;
                z[u] = X[o];
                if (L2) z[u] = z[u] + c2 * L2[o];   // X + (1/mu_2)*lambda_2
            }
        }
        __syncthreads();   // the previous chunk's fragments are read
#pragma unroll
        for (int u = 0; u < kWideChunk / 2; ++u) Zs[((tid >> 7) + 2 * u) * kWideLd + cl] = z[u];
        __syncthreads();
        const int rows4 = (rows + 3) & ~3;   // rows past `rows` are staged as zeros
        for (int r = 0; r < rows4; r += 4) {
            const float *zr = Zs + (r + g) * kWideLd + jl;
            const double fa = (double)zr[16 * wv];
            double fb[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) fb[b] = (double)zr[boff + 16 * b];
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa, fb[b], acc[b], 0, 0, 0);
        }
    }
    // C/D layout of the f64 MFMA: column l & 15, row (l >> 4) + 4 i
    const int npair = nt * (nt + 1) / 2;
    double *out = partial + (int64_t)blockIdx.x * npair * 256;
    const int a = 4 * pa + wv;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int tb = 4 * pb + b;
        if (a < nt && tb < nt && a <= tb) {
            const int pi = a * nt - ((a * (a - 1)) >> 1) + (tb - a);
#pragma unroll
            for (int i = 0; i < 4; ++i) out[(int64_t)pi * 256 + (g + 4 * i) * 16 + jl] = acc[b][i];
        }
    }
}

}  // namespace lrs

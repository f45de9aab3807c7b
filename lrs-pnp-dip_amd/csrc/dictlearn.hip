// Masked dictionary learning (include/lrspnp.h, "Dictionary learning"): the dictionary step of
//   F(D, A) = sum_j 1/2 ||m_j .* (y_j - D a_j)||^2 + lambda ||a_j||_1,   ||d_k||_2 <= 1
// with the coefficients A fixed -- the majorisation-minimisation update of Yaghoobi, Blumensath and
// Davies with the observation mask inside the residual:
//   H = A^T A,  c = max_k sum_l |H_kl|   (Gershgorin: c >= lambda_max(H), the step 1/c is safe)
//   R = m .* (Y - A D^T),  obj = 1/2 ||R||_F^2,  G = R^T A,  u_k = d_k + g_k / c,
//   d_k = u_k / max(1, ||u_k||_2)
// The sparse-coding half of a round is lrs_ista_f32 / lrs_ista_pat_f32, unchanged.
//
// The three products (A D^T: nb x K x n, R^T A: n x nb x K, A^T A: K x nb x K) run on the bf16 matrix
// cores as fp32-accurate split-bf16 products (lrs_split.h): every fp32 operand value is split into its
// three bf16 terms when its tile is written to LDS.  One kernel, k_dl_gemm,
// serves all three through its operand strides; the mask, the subtraction and the squared residual
// are the first product's epilogue.  The two products that sum over the nb blocks are split over
// that sum into fixed chunks whose partials are added in chunk order (fp64), the objective and the
// column norms are fp64 sums in a fixed order: no floating-point atomics, so two runs on the same
// inputs give the same bits.  c is read from device memory; nothing synchronises the host.
#include "lrs_split.h"

namespace lrs {

constexpr int kDlTile = 64;   // output tile per 256-thread workgroup (2 x 2 waves of 32 x 32)
constexpr int kDlK = 32;      // k per step (one MFMA)
// LDS row stride in bf16: 80 B, so the 16 rows of a fragment read (ds_read_b128 at one 16-B k chunk)
// start 20 banks apart and cover the 64 banks once
constexpr int kDlLd = 40;

struct DlGemm {
    const float *A;   // A(m, k) = A[m * sam + k * sak]
    int64_t sam, sak;
    const float *B;   // B(k, n) = B[k * sbk + n * sbn]
    int64_t sbk, sbn;
    int M, N, Kd, kchunk;   // C = A B summed over Kd, chunk z sums [z * kchunk, (z + 1) * kchunk)
    float *C;               // chunk z's partial at C + z * zstride, leading dimension ldc
    int64_t ldc, zstride;
    // residual epilogue: C[m][i] = obs ? Y - acc : 0 for i < n, 0 for n <= i < n_pad (ldc = n_pad)
    const float *Y;
    const uint8_t *obs;
    int n, n_pad;
    double *objp;   // [tile] sum of the tile's squared residuals
};

// the thread's 8 consecutive k of one operand row for the step at k0 (zero outside the operand):
//  KC (k contiguous in memory): row t / 4, k = 8 (t & 3) + 0..7 -- 32 contiguous bytes per thread;
//  else (rows contiguous)     : row t & 63, k = 8 (t >> 6) + 0..7 -- each load coalesced over the lanes
template <bool KC>
__device__ __forceinline__ void dl_load(const float *__restrict__ S, int64_t sx, int64_t sk, int X, int x0, int k0,
                                        int kend, float (&v)[8]) {
    const int t = threadIdx.x;
    const int x = x0 + (KC ? (t >> 2) : (t & 63));
    const int kb = k0 + 8 * (KC ? (t & 3) : (t >> 6));
    if (KC) {
        const float *src = S + (int64_t)x * sx + kb;
        if (x < X && kb + 8 <= kend && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            const float4 a = *reinterpret_cast<const float4 *>(src), b = *reinterpret_cast<const float4 *>(src + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
            v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = (x < X && kb + u < kend) ? src[u] : 0.0f;
        }
    } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = (x < X && kb + u < kend) ? S[(int64_t)(kb + u) * sk + (int64_t)x * sx] : 0.0f;
    }
}

// the three bf16 planes of the 8 values, one 16-B LDS write per plane.  The arithmetic is split_bf16's
// (lrs_split.h) and must follow it; it is spelled out here, hi and mid placed before lo is formed,
// because through split_bf16x8 both k_dl_gemm instantiations schedule these conversions differently
// (same instructions, other order and registers) and the device code is held fixed.
template <bool KC>
__device__ __forceinline__ void dl_store(__bf16 (*T)[kDlTile][kDlLd], const float (&v)[8]) {
    const int t = threadIdx.x;
    const int row = KC ? (t >> 2) : (t & 63), kb = 8 * (KC ? (t & 3) : (t >> 6));
    bf16x8 p0, p1, p2;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = v[e];
        const __bf16 b0 = (__bf16)x;
        const float r1 = x - (float)b0;
        const __bf16 b1 = (__bf16)r1;
        p0[e] = b0;
        p1[e] = b1;
        p2[e] = (__bf16)(r1 - (float)b1);
    }
    *reinterpret_cast<bf16x8 *>(&T[0][row][kb]) = p0;
    *reinterpret_cast<bf16x8 *>(&T[1][row][kb]) = p1;
    *reinterpret_cast<bf16x8 *>(&T[2][row][kb]) = p2;
}

// blockIdx.x = M tile, blockIdx.y = N tile, blockIdx.z = chunk of the summed dimension.
// (the MFMA's lane layout: split_mfma6, lrs_split.h)
template <bool AKC, bool BKC, bool RESID>
__global__ __launch_bounds__(256) void k_dl_gemm(DlGemm g) {
    __shared__ __attribute__((aligned(16))) __bf16 As[3][kDlTile][kDlLd];
    __shared__ __attribute__((aligned(16))) __bf16 Bs[3][kDlTile][kDlLd];
    __shared__ double red[4];
    const int m0 = blockIdx.x * kDlTile, n0 = blockIdx.y * kDlTile;
    const int kbeg = blockIdx.z * g.kchunk, kend = min(g.Kd, kbeg + g.kchunk);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wm = (wv >> 1) * 32, wn = (wv & 1) * 32;
    const int jl = lane & 15, gk = lane >> 4;
    floatx4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = floatx4{0.f, 0.f, 0.f, 0.f};
    float va[8], vb[8];
    dl_load<AKC>(g.A, g.sam, g.sak, g.M, m0, kbeg, kend, va);
    dl_load<BKC>(g.B, g.sbn, g.sbk, g.N, n0, kbeg, kend, vb);
    for (int k0 = kbeg; k0 < kend; k0 += kDlK) {
        dl_store<AKC>(As, va);
        dl_store<BKC>(Bs, vb);
        __syncthreads();
        if (k0 + kDlK < kend) {   // the next step's operands are in flight during the MFMAs
            dl_load<AKC>(g.A, g.sam, g.sak, g.M, m0, k0 + kDlK, kend, va);
            dl_load<BKC>(g.B, g.sbn, g.sbk, g.N, n0, k0 + kDlK, kend, vb);
        }
        bf16x8 fa[2][3], fb[2][3];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                fa[a][p] = *reinterpret_cast<const bf16x8 *>(&As[p][wm + 16 * a + jl][8 * gk]);
                fb[a][p] = *reinterpret_cast<const bf16x8 *>(&Bs[p][wn + 16 * a + jl][8 * gk]);
            }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[a][b] = split_mfma6(fa[a], fb[b], acc[a][b]);
        __syncthreads();
    }
    if constexpr (RESID) {
        double sq = 0.0;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = m0 + wm + 16 * a + 4 * gk + r, i = n0 + wn + 16 * b + jl;
                    if (m < g.M && i < g.n_pad) {
                        const int64_t at = (int64_t)m * g.n_pad + i;
                        float v = 0.0f;
                        if (i < g.n && g.obs[at]) v = g.Y[at] - acc[a][b][r];
                        g.C[at] = v;
                        sq += (double)v * (double)v;
                    }
                }
        // the tile's sum in a fixed order: butterfly over the wave, then the four waves in turn
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off);
        if (lane == 0) red[wv] = sq;
        __syncthreads();
        if (threadIdx.x == 0)
            g.objp[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    } else {
        float *C = g.C + (int64_t)blockIdx.z * g.zstride;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = m0 + wm + 16 * a + 4 * gk + r, nn = n0 + wn + 16 * b + jl;
                    if (m < g.M && nn < g.N) C[(int64_t)m * g.ldc + nn] = acc[a][b][r];
                }
    }
}

// sum of a workgroup's 256 per-thread doubles in a fixed order (a tree over the thread index)
__device__ __forceinline__ double dl_block_sum(double v, double *sm) {
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    const double r = sm[0];
    __syncthreads();
    return r;
}

// *obj = 1/2 * sum of the tile partials (one workgroup, thread t sums tiles t, t + 256, ... in order)
__global__ __launch_bounds__(256) void k_dl_obj(const double *__restrict__ objp, int64_t ntiles, double *obj) {
    __shared__ double sm[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < ntiles; i += 256) s += objp[i];
    s = dl_block_sum(s, sm);
    if (threadIdx.x == 0) *obj = 0.5 * s;
}

// nz[k] = 1 where column k of coefs has a non-zero entry, i.e. H_kk > 0 (nz zeroed before the launch;
// the racing stores all write the same value)
__global__ __launch_bounds__(256) void k_dl_colnz(const float *__restrict__ coefs, int64_t total, int K, int *nz) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
        if (coefs[i] != 0.0f) nz[(int)(i % K)] = 1;
}

// 16 atoms per workgroup, 16 row lanes per atom (a row's 16 atoms are 64 contiguous bytes of D).
//  UPDATE: u_k = d_k + g_k / c with g_k = the chunk partials of R^T A added in chunk order (0 for an
//          atom no block uses), d_k = u_k / max(1, ||u_k||); nothing is written when c is not > 0
//  else  : d_k = d_k / ||d_k|| for the columns with a non-zero norm (columnNormalise.m)
// ||.|| accumulates in fp64: per row lane over its rows in order, then over the 16 lanes in order.
template <bool UPDATE>
__global__ __launch_bounds__(256) void k_dl_atoms(float *__restrict__ D, int n, int K, const float *__restrict__ Gp,
                                                  int nsplit, const int *__restrict__ nz, const double *__restrict__ cptr) {
    __shared__ double sm[16][17];
    const int ka = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int k = blockIdx.x * 16 + ka;
    float cf = 1.0f;
    if (UPDATE) {
        const double c = *cptr;
        if (!(c > 0.0)) return;   // every coefficient is zero: D stays as it is (uniform over the grid)
        cf = (float)c;
    }
    double nrm = 0.0;
    if (k < K) {
        const bool used = UPDATE ? nz[k] != 0 : false;
        for (int i = rl; i < n; i += 16) {
            const int64_t at = (int64_t)i * K + k;
            float u = D[at];
            if (UPDATE) {
                double gs = 0.0;
                if (used)
                    for (int s = 0; s < nsplit; ++s) gs += (double)Gp[(int64_t)s * n * K + at];
                u = u + (float)gs / cf;
                D[at] = u;
            }
            nrm += (double)u * (double)u;
        }
    }
    sm[rl][ka] = nrm;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) tot += sm[r][ka];
    const double nr = sqrt(tot);
    float div;
    if (UPDATE) div = (float)(nr > 1.0 ? nr : 1.0);
    else div = nr > 0.0 ? (float)nr : 1.0f;
    if (k < K && div != 1.0f)
        for (int i = rl; i < n; i += 16) {
            const int64_t at = (int64_t)i * K + k;
            D[at] = D[at] / div;
        }
}

// row k of H = the chunk partials of A^T A added in chunk order, rounded to fp32; rows[k] = the fp64
// sum of |H_kl| over the stored values
__global__ __launch_bounds__(256) void k_dl_hrow(const float *__restrict__ Hp, int nsplit, int K, float *__restrict__ H,
                                                 double *__restrict__ rows) {
    __shared__ double sm[256];
    const int k = blockIdx.x;
    double a = 0.0;
    for (int l = threadIdx.x; l < K; l += 256) {
        double h = 0.0;
        for (int s = 0; s < nsplit; ++s) h += (double)Hp[((int64_t)s * K + k) * K + l];
        const float hf = (float)h;
        H[(int64_t)k * K + l] = hf;
        a += fabs((double)hf);
    }
    a = dl_block_sum(a, sm);
    if (threadIdx.x == 0) rows[k] = a;
}

__global__ __launch_bounds__(256) void k_dl_cmax(const double *__restrict__ rows, int K, double *c) {
    __shared__ double sm[256];
    double m = 0.0;
    for (int l = threadIdx.x; l < K; l += 256) m = fmax(m, rows[l]);
    sm[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *c = sm[0];
}

}  // namespace lrs

using namespace lrs;

namespace {

constexpr int64_t kDlMaxK = 512;
constexpr int64_t kDlMaxNb = (int64_t)1 << 24;
constexpr int64_t kDlMaxNpad = (int64_t)1 << 20;

int64_t dl_tiles(int64_t x) { return (x + kDlTile - 1) / kDlTile; }

// chunks of the sum over the nb blocks: enough workgroups to fill the chip (about 1024), at least 256
// blocks per chunk, at most 64 chunks; a function of the shapes alone, so the summation order is too
void dl_split(int64_t tiles, int64_t kd, int *nsplit, int *kchunk) {
    int64_t s = 1024 / tiles;
    s = s < 1 ? 1 : (s > 64 ? 64 : s);
    const int64_t most = (kd + 255) / 256;
    if (s > most) s = most;
    const int64_t kc = round_up((kd + s - 1) / s, kDlK);
    *kchunk = (int)kc;
    *nsplit = (int)((kd + kc - 1) / kc);
}

struct DlLayout {
    int s2, kc2, s3, kc3;
    int64_t tiles1;
    size_t off_r, off_g, off_objp, off_nz, total_update;
    size_t off_h, off_rows, total_stats;
};

size_t dl_al(size_t x) { return (x + 255) / 256 * 256; }

// the update's buffers (R, the R^T A partials, the objective's tile partials, the used-atom flags) and
// the statistics' (the A^T A partials, the row sums) overlap: each call fills what it reads
DlLayout dl_layout(int64_t n, int64_t n_pad, int64_t K, int64_t nb) {
    DlLayout L;
    dl_split(dl_tiles(n) * dl_tiles(K), nb, &L.s2, &L.kc2);
    dl_split(dl_tiles(K) * dl_tiles(K), nb, &L.s3, &L.kc3);
    L.tiles1 = dl_tiles(nb) * dl_tiles(n_pad);
    size_t o = 0;
    L.off_r = o;
    o = dl_al(o + (size_t)nb * n_pad * sizeof(float));
    L.off_g = o;
    o = dl_al(o + (size_t)L.s2 * n * K * sizeof(float));
    L.off_objp = o;
    o = dl_al(o + (size_t)L.tiles1 * sizeof(double));
    L.off_nz = o;
    o = dl_al(o + (size_t)K * sizeof(int));
    L.total_update = o;
    o = 0;
    L.off_h = o;
    o = dl_al(o + (size_t)L.s3 * K * K * sizeof(float));
    L.off_rows = o;
    o = dl_al(o + (size_t)K * sizeof(double));
    L.total_stats = o;
    return L;
}

int dl_shape(int64_t n, int64_t n_pad, int64_t K, int64_t nb) {
    if (n <= 0 || K <= 0 || nb <= 0 || n_pad < n || n_pad % 16 != 0) return LRS_E_INVALID;
    if (K > kDlMaxK || nb > kDlMaxNb || n_pad > kDlMaxNpad) return LRS_E_UNSUPPORTED;
    return LRS_OK;
}

// R = obs .* (Yb - coefs D^T) into ws and *obj = 1/2 ||R||^2
int dl_residual(const float *Yb, const uint8_t *obs, const float *coefs, const float *D, int64_t n, int64_t n_pad,
                int64_t K, int64_t nb, const DlLayout &L, char *w, double *obj, hipStream_t st) {
    DlGemm g{};
    g.A = coefs; g.sam = K; g.sak = 1;
    g.B = D; g.sbk = 1; g.sbn = K;
    g.M = (int)nb; g.N = (int)n; g.Kd = (int)K; g.kchunk = (int)round_up(K, kDlK);
    g.C = reinterpret_cast<float *>(w + L.off_r); g.ldc = n_pad; g.zstride = 0;
    g.Y = Yb; g.obs = obs; g.n = (int)n; g.n_pad = (int)n_pad;
    g.objp = reinterpret_cast<double *>(w + L.off_objp);
    hipLaunchKernelGGL((k_dl_gemm<true, true, true>), dim3((unsigned)dl_tiles(nb), (unsigned)dl_tiles(n_pad), 1),
                       dim3(256), 0, st, g);
    LRS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_dl_obj, dim3(1), dim3(256), 0, st, g.objp, L.tiles1, obj);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

}  // namespace

extern "C" size_t lrs_dict_workspace(int64_t n, int64_t n_pad, int64_t K, int64_t nb) {
    if (dl_shape(n, n_pad, K, nb) != LRS_OK) return 0;
    const DlLayout L = dl_layout(n, n_pad, K, nb);
    return L.total_update > L.total_stats ? L.total_update : L.total_stats;
}

extern "C" int lrs_dict_stats_f32(const float *coefs, int64_t nb, int64_t K, float *H, double *c, void *ws,
                                  size_t ws_bytes, void *stream) {
    if (!coefs || !H || !c) return LRS_E_INVALID;
    const int rc = dl_shape(16, 16, K, nb);
    if (rc != LRS_OK) return rc;
    const DlLayout L = dl_layout(16, 16, K, nb);
    if (!ws || ws_bytes < L.total_stats) return LRS_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char *w = static_cast<char *>(ws);
    DlGemm g{};
    g.A = coefs; g.sam = 1; g.sak = K;
    g.B = coefs; g.sbk = K; g.sbn = 1;
    g.M = (int)K; g.N = (int)K; g.Kd = (int)nb; g.kchunk = L.kc3;
    g.C = reinterpret_cast<float *>(w + L.off_h); g.ldc = K; g.zstride = K * K;
    hipLaunchKernelGGL((k_dl_gemm<false, false, false>), dim3((unsigned)dl_tiles(K), (unsigned)dl_tiles(K), (unsigned)L.s3),
                       dim3(256), 0, st, g);
    LRS_CHECK_LAUNCH();
    double *rows = reinterpret_cast<double *>(w + L.off_rows);
    hipLaunchKernelGGL(k_dl_hrow, dim3((unsigned)K), dim3(256), 0, st, g.C, L.s3, (int)K, H, rows);
    LRS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_dl_cmax, dim3(1), dim3(256), 0, st, rows, (int)K, c);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

extern "C" int lrs_dict_update_f32(const float *Yb, const uint8_t *obs, const float *coefs, float *D, int64_t n,
                                   int64_t n_pad, int64_t K, int64_t nb, const double *c, int n_inner, double *obj,
                                   void *ws, size_t ws_bytes, void *stream) {
    if (!Yb || !obs || !coefs || !D || !c || !obj || n_inner < 0) return LRS_E_INVALID;
    const int rc = dl_shape(n, n_pad, K, nb);
    if (rc != LRS_OK) return rc;
    const DlLayout L = dl_layout(n, n_pad, K, nb);
    if (!ws || ws_bytes < L.total_update) return LRS_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char *w = static_cast<char *>(ws);
    int *nz = reinterpret_cast<int *>(w + L.off_nz);
    hipError_t e = hipMemsetAsync(nz, 0, (size_t)K * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    const int64_t total = nb * K;
    const int64_t nzgrid = (total + 255) / 256;
    hipLaunchKernelGGL(k_dl_colnz, dim3((unsigned)(nzgrid < 2048 ? nzgrid : 2048)), dim3(256), 0, st, coefs, total, (int)K,
                       nz);
    LRS_CHECK_LAUNCH();
    DlGemm g{};   // G = R^T coefs, chunked over the blocks
    g.A = reinterpret_cast<const float *>(w + L.off_r); g.sam = 1; g.sak = n_pad;
    g.B = coefs; g.sbk = K; g.sbn = 1;
    g.M = (int)n; g.N = (int)K; g.Kd = (int)nb; g.kchunk = L.kc2;
    g.C = reinterpret_cast<float *>(w + L.off_g); g.ldc = K; g.zstride = n * K;
    for (int it = 0; it < n_inner; ++it) {
        int r = dl_residual(Yb, obs, coefs, D, n, n_pad, K, nb, L, w, obj + it, st);
        if (r != LRS_OK) return r;
        hipLaunchKernelGGL((k_dl_gemm<false, false, false>), dim3((unsigned)dl_tiles(n), (unsigned)dl_tiles(K), (unsigned)L.s2),
                           dim3(256), 0, st, g);
        LRS_CHECK_LAUNCH();
        hipLaunchKernelGGL((k_dl_atoms<true>), dim3((unsigned)((K + 15) / 16)), dim3(256), 0, st, D, (int)n, (int)K, g.C,
                           L.s2, nz, c);
        LRS_CHECK_LAUNCH();
    }
    return dl_residual(Yb, obs, coefs, D, n, n_pad, K, nb, L, w, obj + n_inner, st);
}

extern "C" int lrs_dict_normalise_f32(float *D, int64_t n, int64_t K, void *stream) {
    if (!D || n <= 0 || K <= 0) return LRS_E_INVALID;
    if (K > kDlMaxK || n > kDlMaxNpad) return LRS_E_UNSUPPORTED;
    hipLaunchKernelGGL((k_dl_atoms<false>), dim3((unsigned)((K + 15) / 16)), dim3(256), 0, (hipStream_t)stream, D, (int)n,
                       (int)K, nullptr, 0, nullptr, nullptr);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

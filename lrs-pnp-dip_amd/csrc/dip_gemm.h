// Split-bf16 GEMM and implicit-GEMM convolution for the DIP engine (gfx950).
//
// C[M][N] = op(A)[M][K] op(B)[K][N] in fp32 accuracy on the bf16 matrix cores (lrs_split.h): every
// fp32 operand value is split into its three bf16 terms ONCE, when its tile is written to LDS, and
// each 16x16 output tile accumulates the six-product chain (split_mfma6) into fp32.
//
// Tile: 128 x 128 per 256-thread workgroup (2 x 2 waves of 64 x 64 = 4 x 4 MFMA tiles), 32 k
// per step.  LDS holds the three bf16 planes of both operands k-contiguous, 64 B rows with the
// 16-B chunk index XOR-swizzled by (row >> 1) & 3, so a lane's 8-k fragment is one conflict-free
// ds_read_b128.  One LDS stage, the next step's global loads in registers during the MFMAs,
// 2-3 workgroups per CU.  gridDim.z > 1 = split-K as in k_gemm.
//
// Operands come from loaders: dense fp32 matrices (split at the LDS store), conv weights
// pre-split into bf16 planes once per step (k_wprep: no split work in the GEMM), or the implicit
// im2col of a conv (reflection / zero padding, stride and the nearest x2 upsample folded into
// LDS offset tables, buffer loads with range-checked zero fill), so no conv direction
// materialises a col matrix (the reference's ReflectionPad2d + Conv2d,
// lipschitz_constraint_layer.py:65-78, common.py:73-121).
#pragma once

#include "lrs_dip.h"
#include "lrs_split.h"
#include "dip_kernels.h"   // GemmArgs

namespace lrs {

constexpr int kS3K = 32;

// LDS image of one operand: [plane][row 0..127][32 k] bf16, chunk (8 k) swizzled per row
struct S3Tile {
    __bf16 v[3][128][kS3K];
};

// chunk ^ ((row >> 1) & 3): conflict-free for the CDNA4 LDS lane groups (MI355X_MICROARCH.md §LDS)
// of both sides -- the fragment reads (ds_read_b128: groups {0-3,12-15,20-27}, ... of 16 lanes over
// 64 banks: rows base + (l & 15), chunk l >> 4) and the tile stores (ds_write_b128: 8 contiguous
// lanes over 32 banks: 8 consecutive rows at one chunk, or 4 rows x 2 chunks).  The previous
// (row >> 2) & 3 was conflict-free only for 16-lane groups {0-15}, ...: measured 8.3M bank-conflict
// cycles per 196^2 forward conv launch (SQ_LDS_BANK_CONFLICT).  Found by exhaustive search over
// f(row mod 16) (tools: DESIGN.md §4).
__device__ __forceinline__ int s3_chunk(int row, int chunk) { return chunk ^ ((row >> 1) & 3); }

// thread -> (row, first k) of the 16 values it loads per step:
//  KC (operand stored k-contiguous): row = t / 2, k = 16 (t & 1) + 0..15
//  else (stored row-contiguous)    : row = t & 127, k = 16 (t >> 7) + 0..15
// (measured: a 2-k x 8-row KC arrangement with 16 lanes per row is slower, 2-20 %)
template <bool KC>
__device__ __forceinline__ int s3_row() { return KC ? (threadIdx.x >> 1) : (threadIdx.x & 127); }
template <bool KC>
__device__ __forceinline__ int s3_kb() { return KC ? 16 * (threadIdx.x & 1) : 16 * (threadIdx.x >> 7); }

template <bool KC>
__device__ __forceinline__ void s3_store(S3Tile &T, const float (&v)[16]) {
    const int row = s3_row<KC>(), c0 = s3_kb<KC>() >> 3;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        bf16x8 p0, p1, p2;
        split_bf16x8(&v[8 * h], p0, p1, p2);
        const int ch = s3_chunk(row, c0 + h) * 8;
        *reinterpret_cast<bf16x8 *>(&T.v[0][row][ch]) = p0;
        *reinterpret_cast<bf16x8 *>(&T.v[1][row][ch]) = p1;
        *reinterpret_cast<bf16x8 *>(&T.v[2][row][ch]) = p2;
    }
}

__device__ __forceinline__ void s3_frag(const S3Tile &T, int row, int gk, bf16x8 (&f)[3]) {
    const int ch = s3_chunk(row, gk) * 8;
#pragma unroll
    for (int p = 0; p < 3; ++p) f[p] = *reinterpret_cast<const bf16x8 *>(&T.v[p][row][ch]);
}

// ---- loaders ---------------------------------------------------------------------------------
// Each provides: static constexpr bool kc; setup(x0, smem, cls) once per workgroup (before the first
// barrier); load(x0, k0, kend, v) the thread's 16 values of the step starting at k0 (zero past
// kend or past the operand's row count).

// Dense operand: KC = stored [x][k] (leading dimension ld), else stored [k][x].
template <bool KC>
struct LdDense {
    static constexpr bool kc = KC;
    static constexpr bool pre = false;
    const float *S;
    int ld, X;
    __device__ __forceinline__ void setup(int, int *, int) {}
    __device__ __forceinline__ void load(int x0, int k0, int kend, float (&v)[16]) const {
        const int x = x0 + s3_row<KC>(), kb = k0 + s3_kb<KC>();
        if (KC) {
            const float *src = S + (int64_t)x * ld + kb;
            if (x < X && kb + 16 <= kend && ((reinterpret_cast<uintptr_t>(src) & 15) == 0)) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 f = *reinterpret_cast<const float4 *>(src + 4 * q);
                    v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
                }
            } else {
#pragma unroll
                for (int u = 0; u < 16; ++u) v[u] = (x < X && kb + u < kend) ? src[u] : 0.0f;
            }
        } else {
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = (x < X && kb + u < kend) ? S[(int64_t)(kb + u) * ld + x] : 0.0f;
        }
    }
};

// source index of padded / upsampled coordinate u (extent n upsampled), -1 for a zero pad
__host__ __device__ __forceinline__ int conv_src(int u, int n, int mode, int up) {
    if (mode == LRS_PAD_REFLECT) {
        u = u < 0 ? -u : u;
        u = u >= n ? 2 * (n - 1) - u : u;
    } else if (u < 0 || u >= n) {
        return -1;
    }
    return up ? (u >> 1) : u;
}

// ---- implicit-GEMM conv operands --------------------------------------------------------------
// The tap tables below are built by k_gemm_s3's 256 threads as thread t -> table column t & 127 (the
// workgroup's pixel), taps t >> 7, t >> 7 + 2, ...: the pixel's coordinates take one division per
// thread, a tap's (ky, kx) none (k <= 4, the effective 4 x 4 data-gradient kernel included; the
// per-entry divisions cost ~1.8 us per workgroup).
__device__ __forceinline__ int s3_tap_y(int kyx, int k) {
    return kyx >= 3 * k ? 3 : (kyx >= 2 * k ? 2 : (kyx >= k ? 1 : 0));
}
// The conv's K index is tap-major, r = kyx * Cp + c (kyx = ky * k + kx, c < Cp = Cin rounded up to
// 16, channels >= Cin are zero), so the 16 consecutive k a thread loads share one tap: their
// source offset is one LDS table entry and the 16 channels are a scalar stride apart.  Sources
// are read through buffer loads (32-bit offsets, range-checked): a table entry kOob marks a zero
// pad / out-of-range pixel and the hardware returns 0 for it, so no per-value select remains.
constexpr int kOob = 0x7FFFFFF0;   // >= every buffer's byte count (host checks < kOob)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t s3_rsrc(const void *p, int bytes) {
    const uint64_t a = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    const void *u = reinterpret_cast<const void *>(((uint64_t)hi << 32) | lo);
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(u), 0, __builtin_amdgcn_readfirstlane(bytes),
                                             0x00020000);
}

__device__ __forceinline__ float s3_bload(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}

// The NV channel planes c0 .. c0 + NV - 1 (plane stride pb bytes) at one tap's offsets vo, without a
// branch or a mask: every load is issued, a channel c >= nc reads channel nc - 1.  The values that
// are not the operand's -- padding channels, and the k groups past a split's end (whose callers
// read tap 0) -- meet zero weights: every implicit-GEMM B loader is paired with LdPre, whose planes
// are zero at ci >= Cin (co >= Cout) and which reads zeros past kend, so they add exact zeros.
// Written as "c < nc ? load : 0" (or with a mask applied to the loaded bits) the compiler branched
// around each load or waited for it right away, and its wait-count pass, meeting paths with
// different loads in flight at the GEMM's loop head, drained them all there (s_waitcnt vmcnt(0)
// every k-step: the prefetch two steps ahead was lost; tools/micro/gemm_phase).
template <int NV>
__device__ __forceinline__ void s3_bload_chans(__amdgpu_buffer_rsrc_t r, int vo, int c0, int nc, int pb, float (&v)[NV]) {
#pragma unroll
    for (int u = 0; u < NV; ++u) v[u] = s3_bload(r, vo, min(c0 + u, nc - 1) * pb);
}

// Pre-split operand (the conv weights, split into bf16 planes by k_wprep): plane p of row x at
// P + p * pstride + x * ld, k contiguous.  Loads go straight to the LDS image (no split).
struct RegP {
    uint4 h[3][2];
};

struct LdPre {
    static constexpr bool kc = true;
    static constexpr bool pre = true;
    const __bf16 *P;
    int64_t pstride;
    int ld, X;
    int64_t cstride = 0;   // parity-class GEMMs: class cls reads the planes at P + cls * cstride
    __device__ __forceinline__ void setup(int, int *, int cls) { P += cls * cstride; }
    // buffer loads, branch-free (s3_bload_chans): a row past X or a k group past kend reads at kOob
    // (zeros); the planes' bytes are < kOob (k_conv_prep's 2^31 / 3 element limit)
    __device__ __forceinline__ void load(int x0, int k0, int kend, RegP &r) const {
        const int x = x0 + s3_row<true>(), kb = k0 + s3_kb<true>();
        const bool ok = x < X && kb < kend;   // K and kend are multiples of 16
        const __amdgpu_buffer_rsrc_t rs = s3_rsrc(P, (int)(6 * pstride));
        const int vo = ok ? 2 * (x * ld + kb) : kOob;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            r.h[p][0] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, (int)(2 * p * pstride), 0));
            r.h[p][1] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, (int)(2 * p * pstride) + 16, 0));
        }
    }
};

__device__ __forceinline__ void s3_store_pre(S3Tile &T, const RegP &r) {
    const int row = s3_row<true>(), c0 = s3_kb<true>() >> 3;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ch = s3_chunk(row, c0 + h) * 8;
#pragma unroll
        for (int p = 0; p < 3; ++p) *reinterpret_cast<uint4 *>(&T.v[p][row][ch]) = r.h[p][h];
    }
}

// load() of the four tap-table B loaders below (table tab [taps][128], K index tap * Cp + channel): the
// step's tap and first channel, then the 16 channel planes (nc valid, pb bytes apart) of source S at the
// thread's table entry.
__device__ __forceinline__ void s3_tap_load(const float *S, int sbytes, const int *tab, int Cp, int nc, int pb, int k0,
                                            int kend, float (&v)[16]) {
    const int r0 = __builtin_amdgcn_readfirstlane(k0 + s3_kb<false>());
    const int rr = r0 < kend ? r0 : 0,   // past the chunk: tap 0 (meets zero weights)
              kyx = rr / Cp, c0 = rr - kyx * Cp;
    const __amdgpu_buffer_rsrc_t rs = s3_rsrc(S, sbytes);
    s3_bload_chans(rs, tab[kyx * 128 + s3_row<false>()], c0, nc, pb, v);
}

// Forward B: col[r][p] (k = r tap-major, x = output pixel p).  Table [kk][128] of the
// workgroup's pixels' source byte offsets within a channel plane.
struct LdFwdTM {
    static constexpr bool kc = false;
    static constexpr bool pre = false;
    const float *X;
    int xbytes;
    ConvGeom g;
    int Cp;
    int *tab;
    __device__ __forceinline__ void setup(int x0, int *smem, int) {
        tab = smem;
        const int kk = g.k * g.k, r = threadIdx.x & 127, p = x0 + r;
        const bool in = p < g.Ho * g.Wo;
        const int oy = in ? p / g.Wo : 0, ox = p - oy * g.Wo;
        for (int kyx = threadIdx.x >> 7; kyx < kk; kyx += 2) {
            const int ky = s3_tap_y(kyx, g.k), kx = kyx - ky * g.k;
            const int sy = conv_src(oy * g.stride + ky - g.pad, g.Hu, g.pad_mode, g.up);
            const int sx = conv_src(ox * g.stride + kx - g.pad, g.Wu, g.pad_mode, g.up);
            tab[kyx * 128 + r] = (in && sy >= 0 && sx >= 0) ? 4 * (sy * g.Ws + sx) : kOob;
        }
    }
    __device__ __forceinline__ void load(int, int k0, int kend, float (&v)[16]) const {
        s3_tap_load(X, xbytes, tab, Cp, g.Cin, g.Hs * g.Ws * 4, k0, kend, v);
    }
};

// Data-gradient B (stride 1): gy at (iy - ky, ix - kx) over the padded, upsampled domain
// q = (iy, ix); k = kyx * Cop + co.  Table [kk][128] of the workgroup's q.
struct LdDgradTM {
    static constexpr bool kc = false;
    static constexpr bool pre = false;
    const float *GY;
    int gbytes;
    ConvGeom g;
    int Cout, Cop;
    int *tab;
    __device__ __forceinline__ void setup(int x0, int *smem, int) {
        tab = smem;
        const int kk = g.k * g.k, Wp = g.Wu + 2 * g.pad, r = threadIdx.x & 127, q = x0 + r;
        const bool in = q < (g.Hu + 2 * g.pad) * Wp;
        const int iy = in ? q / Wp : 0, ix = q - iy * Wp;
        for (int kyx = threadIdx.x >> 7; kyx < kk; kyx += 2) {
            const int ky = s3_tap_y(kyx, g.k), kx = kyx - ky * g.k;
            const int oy = iy - ky, ox = ix - kx;
            tab[kyx * 128 + r] = (in && oy >= 0 && oy < g.Ho && ox >= 0 && ox < g.Wo) ? 4 * (oy * g.Wo + ox) : kOob;
        }
    }
    __device__ __forceinline__ void load(int, int k0, int kend, float (&v)[16]) const {
        s3_tap_load(GY, gbytes, tab, Cop, Cout, g.Ho * g.Wo * 4, k0, kend, v);
    }
};

// Lane-per-pixel staging of a weight gradient's col^T tile (128 rows r x 32 pixels per k-step):
// wave w owns rows 32 w .. 32 w + 31, lane l pixel l & 31 of rows 32 w + 2 u + (l >> 5), u < 16, so
// each load instruction reads 2 x 32 consecutive pixels of one channel plane (coalesced), and the
// values go to the row-major LDS image as single bf16 writes.  Rows = (channel, tap) pairs, ntap
// taps per channel; tab = the step's [ntap][32] source offsets (kOob = zero).
__device__ __forceinline__ int wlp_row(int u) { return 32 * (threadIdx.x >> 6) + 2 * u + ((threadIdx.x >> 5) & 1); }

__device__ __forceinline__ void wlp_load(const float *X, int xbytes, int plane_bytes, int nrows, int ntap, int x0,
                                         const int *tab, float (&v)[16]) {
    const __amdgpu_buffer_rsrc_t rs = s3_rsrc(X, xbytes);
    const int pl = threadIdx.x & 31;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int r = x0 + wlp_row(u), c = r / ntap, tap = r - c * ntap;
        v[u] = s3_bload(rs, tab[tap * 32 + pl] + (r < nrows ? c * plane_bytes : kOob), 0);
    }
}

__device__ __forceinline__ void wlp_store(S3Tile &T, const float (&v)[16]) {
    const int k = threadIdx.x & 31;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int row = wlp_row(u), at = s3_chunk(row, k >> 3) * 8 + (k & 7);
        const Bf16Split q = split_bf16(v[u]);
        T.v[0][row][at] = q.b0;
        T.v[1][row][at] = q.b1;
        T.v[2][row][at] = q.b2;
    }
}

// Weight-gradient B: col^T, x = r = c * kk + kyx (dW's own column order: a wave's 32 rows are
// ~4 channels x all taps, whose gathers share cache lines), k = output pixel.  The thread's row
// is fixed; the step's 32 pixels x kk taps are tabulated one step ahead (prepare,
// double-buffered).  Rows past Cin * kk read at kOob (zeros).
struct LdWgradTM {
    static constexpr bool kc = true;
    static constexpr bool pre = false;
    static constexpr bool lanepix = true;   // wlp_load / wlp_store (coalesced gathers)
    const float *X;
    int xbytes;
    ConvGeom g;
    int *tab;   // [2][kk][32]
    int x0;
    __device__ __forceinline__ void setup(int x0_, int *smem, int) {
        tab = smem;
        x0 = x0_;
    }
    __device__ __forceinline__ void prepare(int k0, int kend, int b) const {
        const int kk = g.k * g.k;
        for (int i = threadIdx.x; i < kk * 32; i += blockDim.x) {
            const int kyx = i >> 5, p = k0 + (i & 31);
            int o = kOob;
            if (p < kend) {
                const int oy = p / g.Wo, ox = p - oy * g.Wo, ky = kyx / g.k, kx = kyx - ky * g.k;
                const int sy = conv_src(oy * g.stride + ky - g.pad, g.Hu, g.pad_mode, g.up);
                const int sx = conv_src(ox * g.stride + kx - g.pad, g.Wu, g.pad_mode, g.up);
                if (sy >= 0 && sx >= 0) o = 4 * (sy * g.Ws + sx);
            }
            tab[b * 9 * 32 + i] = o;
        }
    }
    __device__ __forceinline__ void load(int, int, int, float (&v)[16], int b) const {
        wlp_load(X, xbytes, g.Hs * g.Ws * 4, g.Cin * g.k * g.k, g.k * g.k, x0, tab + b * 9 * 32, v);
    }
};

// ---- upsampled 3 x 3 convs by output parity class -------------------------------------------
// conv3x3(ReflectionPad2d(1)(Upsample2x(x))) (my_Lipschitz_Unet.py:83-94): output pixel
// (2a + i, 2b + j) reads source rows clamp(a + ey + i - 1), ey in {0, 1}, through the tap sets
// T(i, ey) = {0} {1, 2} (i = 0) or {0, 1} {2} (i = 1), and likewise the columns: the reflection of the
// upsampled border is a clamp on the source grid.  Per class the conv is a 2 x 2 conv of x with
// summed ("effective") weights (k_conv_prep's upc planes): 16 / 9 of the taps of one class, so the
// four classes cost 4 / 9 of the direct product over the upsampled grid.

__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// Forward B of class cls = 2 i + j: col[e * Cp + c][n], n = source pixel (a, b), e = 2 ey + ex:
// x[c] at (clamp(a + ey + i - 1), clamp(b + ex + j - 1)).  Table [4][128].
struct LdUpFwdTM {
    static constexpr bool kc = false;
    static constexpr bool pre = false;
    const float *X;
    int xbytes;
    ConvGeom g;
    int Cp;
    int *tab;
    __device__ __forceinline__ void setup(int x0, int *smem, int cls) {
        tab = smem;
        const int i = cls >> 1, j = cls & 1, r = threadIdx.x & 127, n = x0 + r;
        const bool in = n < g.Hs * g.Ws;
        const int a = in ? n / g.Ws : 0, b = n - a * g.Ws;
        for (int e = threadIdx.x >> 7; e < 4; e += 2)
            tab[e * 128 + r] = in ? 4 * (clampi(a + (e >> 1) + i - 1, g.Hs) * g.Ws + clampi(b + (e & 1) + j - 1, g.Ws)) : kOob;
    }
    __device__ __forceinline__ void load(int, int k0, int kend, float (&v)[16]) const {
        s3_tap_load(X, xbytes, tab, Cp, g.Cin, g.Hs * g.Ws * 4, k0, kend, v);
    }
};

// Data-gradient B of the same conv over the source grid extended by one pixel on each side
// (n = (qy + 1)(Ws + 2) + qx + 1, qy in [-1, Hs], qx in [-1, Ws]; k_fold_pad in kPadClamp mode adds
// the outside ring back onto the border): k = (4 cls + e) Cop + co, dL/dz[co] at
// (2a + i, 2b + j) with a = qy - ey - i + 1, b = qx - ex - j + 1 when inside.  Table [16][128].
struct LdUpDgradTM {
    static constexpr bool kc = false;
    static constexpr bool pre = false;
    const float *GY;
    int gbytes;
    ConvGeom g;
    int Cout, Cop;
    int *tab;
    __device__ __forceinline__ void setup(int x0, int *smem, int) {
        tab = smem;
        const int We = g.Ws + 2, r = threadIdx.x & 127, n = x0 + r;
        const bool in = n < (g.Hs + 2) * We;
        const int qy = (in ? n / We : 0) - 1, qx = n - (qy + 1) * We - 1;
        for (int ce = threadIdx.x >> 7; ce < 16; ce += 2) {
            const int cl = ce >> 2, e = ce & 3, i = cl >> 1, j = cl & 1;
            const int a = qy - (e >> 1) - i + 1, b = qx - (e & 1) - j + 1;
            tab[ce * 128 + r] = (in && a >= 0 && a < g.Hs && b >= 0 && b < g.Ws) ? 4 * ((2 * a + i) * g.Wo + 2 * b + j) : kOob;
        }
    }
    __device__ __forceinline__ void load(int, int k0, int kend, float (&v)[16]) const {
        s3_tap_load(GY, gbytes, tab, Cop, Cout, g.Ho * g.Wo * 4, k0, kend, v);
    }
};

// Weight gradient of the same conv by output parity class cls (gridDim.z = 4 classes x split-K):
// dWE_cls[co][c * 4 + e] = sum over source pixels (a, b) of dL/dz[co] at (2a + i, 2b + j) times x[c]
// at (clamp(a + ey + i - 1), clamp(b + ex + j - 1)); the classes are stacked in the output
// ([split][cls][Cout][4 Cin], GemmArgs cls_wo = 0) and k_upc_wgrad_combine sums them into dW.
// A: dL/dz at the class's output pixels, k = source pixel (16 consecutive per thread).
struct LdGzCls {
    static constexpr bool kc = true;
    static constexpr bool pre = false;
    static constexpr bool lanepix = true;   // lane = source pixel (wlp_store), as the col^T side
    const float *GZ;
    int Hs, Ws, Wo, M;
    int cls;
    __device__ __forceinline__ void setup(int, int *, int c) { cls = c; }
    __device__ __forceinline__ void load(int x0, int k0, int kend, float (&v)[16]) const {
        const int k = k0 + (threadIdx.x & 31), i = cls >> 1, j = cls & 1;
        const int a = k / Ws, b = k - a * Ws;
        const int po = (2 * a + i) * Wo + 2 * b + j;
        const __amdgpu_buffer_rsrc_t rs = s3_rsrc(GZ, M * 4 * Hs * Ws * 4);
        // the row offset differs between the wave's two halves: in the VGPR offset, not the SGPR one
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int row = x0 + wlp_row(u);
            v[u] = s3_bload(rs, (k < kend && row < M) ? 4 * po + row * (4 * Hs * Ws * 4) : kOob, 0);
        }
    }
};

// B: col^T of the class, x = r = c * 4 + e, k = source pixel; the step's 32 pixels x 4 taps
// tabulated one step ahead (double-buffered, as LdWgradTM).
struct LdWgradCls {
    static constexpr bool kc = true;
    static constexpr bool pre = false;
    static constexpr bool lanepix = true;
    const float *X;
    int xbytes;
    ConvGeom g;
    int *tab;   // [2][4][32]
    int x0, cls;
    __device__ __forceinline__ void setup(int x0_, int *smem, int c) {
        tab = smem;
        x0 = x0_;
        cls = c;
    }
    __device__ __forceinline__ void prepare(int k0, int kend, int b) const {
        const int i = cls >> 1, j = cls & 1;
        for (int idx = threadIdx.x; idx < 4 * 32; idx += blockDim.x) {
            const int e = idx >> 5, p = k0 + (idx & 31);
            int o = kOob;
            if (p < kend) {
                const int a = p / g.Ws, bb = p - a * g.Ws;
                o = 4 * (clampi(a + (e >> 1) + i - 1, g.Hs) * g.Ws + clampi(bb + (e & 1) + j - 1, g.Ws));
            }
            tab[b * 4 * 32 + idx] = o;
        }
    }
    __device__ __forceinline__ void load(int, int, int, float (&v)[16], int b) const {
        wlp_load(X, xbytes, g.Hs * g.Ws * 4, 4 * g.Cin, 4, x0, tab + b * 4 * 32, v);
    }
};

// dW[co][c][ky][kx] = (sum over the 4 classes of dWE_cls[co][c * 4 + e(cls, ky, kx)], each summed over
// the nsplit splits in k_gemm_reduce's order) / *div: the chain rule through upc_weight's sums.
__global__ void k_upc_wgrad_combine(const float *__restrict__ part, int nsplit, int Cout, int Cin,
                                    const float *div, float *__restrict__ gw) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, n = (int64_t)Cout * Cin * 9;
    if (idx >= n) return;
    const int tap = (int)(idx % 9), c = (int)((idx / 9) % Cin), co = (int)(idx / (9 * (int64_t)Cin));
    const int ky = tap / 3, kx = tap - 3 * ky;
    const int64_t MN = (int64_t)Cout * 4 * Cin;
    float tot = 0.0f;
    for (int cl = 0; cl < 4; ++cl) {
        const int i = cl >> 1, j = cl & 1;
        const int ey = i == 0 ? (ky == 0 ? 0 : 1) : (ky == 2 ? 1 : 0), ex = j == 0 ? (kx == 0 ? 0 : 1) : (kx == 2 ? 1 : 0);
        const int64_t off = (int64_t)cl * MN + (int64_t)co * 4 * Cin + c * 4 + 2 * ey + ex;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int z0 = 0; z0 < nsplit; z0 += 8) {
            float p[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) p[e] = z0 + e < nsplit ? part[(int64_t)(z0 + e) * 4 * MN + off] : 0.0f;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (z0 + e < nsplit) acc[e] += p[e];
        }
        tot = tot + (((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7])));
    }
    if (div) tot = tot / *div;
    gw[idx] = tot;
}

template <class L>
struct HasPrepare {
    static constexpr bool value = false;
};
template <class L, class = void>
struct LanePix {
    static constexpr bool value = false;
};
template <class L>
struct LanePix<L, std::void_t<decltype(L::lanepix)>> {
    static constexpr bool value = L::lanepix;
};

template <>
struct HasPrepare<LdWgradTM> {
    static constexpr bool value = true;
};
template <>
struct HasPrepare<LdWgradCls> {
    static constexpr bool value = true;
};

constexpr int kS3TabInts = 16 * 128;  // k <= 4 (the 4 x 4 effective kernel of an upsampled 3 x 3 conv's data gradient)

// The LDS of one k_gemm_s3 workgroup: both operand images (one object: the epilogue reuses them as a
// 4 x 32 x 68-float staging area) and the loaders' tap tables.
struct S3Smem {
    struct {
        S3Tile a, b;
    } ab;
    int tab[kS3TabInts];
};
static_assert(sizeof(S3Tile) * 2 >= 4 * 32 * 68 * sizeof(float), "epilogue staging fits the operand images");

// One workgroup of the split-bf16 GEMM.  (gx, gy, gz): the GEMM's own grid (N tiles, M tiles, classes x
// split-K); L: this workgroup's linear index in it, which the hardware deals to XCD L % 8.
// (Kept apart from k_gemm_s3, its only caller: written into the kernel, the same statements compile to
// different code in every instantiation -- other register counts in five.)
template <class LA, class LB>
__device__ __forceinline__ void gemm_s3_body(const GemmArgs &g, LA la, LB lb, S3Smem &sm, int L, unsigned gx,
                                             unsigned gy, unsigned gz) {
    auto &ab = sm.ab;
    S3Tile &As = ab.a, &Bs = ab.b;
    int *tab = sm.tab;
    // XCD-aware tile order: the hardware deals workgroup L to XCD L % 8 (placement matters for
    // speed only), so consecutive logical tiles -- neighbouring pixel tiles that share input rows,
    // the N-tiles of one split-K chunk that share its A rows -- are given to one XCD and meet in
    // its L2 instead of being fetched from HBM by all eight
    const int T = gx * gy * gz;
    const int xcd = L & 7, q8 = T >> 3, r8 = T & 7;
    const int j = xcd * q8 + min(xcd, r8) + (L >> 3);
    const int bx = j % gx, byz = j / gx, by = byz % gy, bz = byz / gy;
    const int m0 = by * 128, n0 = bx * 128;
    const int ncls = g.ncls > 1 ? g.ncls : 1, cls = bz % ncls, kz = bz / ncls;   // parity class, split
    const int kbeg = kz * g.kchunk;
    const int kend = min(g.K, kbeg + g.kchunk);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wm = (wv >> 1) * 64, wn = (wv & 1) * 64;
    const int jl = lane & 15, gk = lane >> 4;
    constexpr bool PREP = HasPrepare<LB>::value;
    la.setup(m0, tab, cls);
    RegP pa;   // LA::pre: the weight planes
    if constexpr (!PREP && LA::pre) {   // the first weight planes are in flight while the tables are built
        la.load(m0, kbeg, kend, pa);
        __builtin_amdgcn_sched_barrier(0);
    }
    lb.setup(n0, tab, cls);
    if constexpr (PREP) lb.prepare(kbeg, kend, 0);
    __syncthreads();
    floatx4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = floatx4{0.f, 0.f, 0.f, 0.f};
    float va[16], vb[16];
    static_assert(!LB::pre, "B is never pre-split");
    auto mma = [&]() {
        bf16x8 fb[4][3];
#pragma unroll
        for (int b = 0; b < 4; ++b) s3_frag(Bs, wn + 16 * b + jl, gk, fb[b]);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            bf16x8 fa[3];
            s3_frag(As, wm + 16 * a + jl, gk, fa);
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = split_mfma6(fa, fb[b], acc[a][b]);
        }
    };
    if constexpr (PREP) {
        if constexpr (LA::pre) la.load(m0, kbeg, kend, pa);
        else la.load(m0, kbeg, kend, va);
        lb.load(n0, kbeg, kend, vb, 0);
        int tb = 0;
        for (int k0 = kbeg; k0 < kend; k0 += kS3K) {
            if constexpr (LA::pre) s3_store_pre(As, pa);
            else if constexpr (LanePix<LA>::value) wlp_store(As, va);
            else s3_store<LA::kc>(As, va);
            if constexpr (LanePix<LB>::value) wlp_store(Bs, vb);
            else s3_store<LB::kc>(Bs, vb);
            if (k0 + kS3K < kend) lb.prepare(k0 + kS3K, kend, tb ^ 1);
            __syncthreads();
            if (k0 + kS3K < kend) {
                if constexpr (LA::pre) la.load(m0, k0 + kS3K, kend, pa);
                else la.load(m0, k0 + kS3K, kend, va);
                lb.load(n0, k0 + kS3K, kend, vb, tb ^ 1);
            }
            tb ^= 1;
            mma();
            __syncthreads();
        }
    } else {
        // the B operand's loads two steps ahead (register sets vb / vb1, the loop unrolled by two),
        // the A operand's one step (the weight planes hit L2; two would spill): with one wave per
        // SIMD a single step of prefetch left the implicit-GEMM gathers exposed behind the MFMAs
        float vb1[16];
        auto ldA = [&](int k0) {
            if constexpr (LA::pre) la.load(m0, k0, kend, pa);
            else la.load(m0, k0, kend, va);
        };
        auto st = [&](const float (&b)[16]) {
            if constexpr (LA::pre) s3_store_pre(As, pa);
            else if constexpr (LanePix<LA>::value) wlp_store(As, va);
            else s3_store<LA::kc>(As, va);
            if constexpr (LanePix<LB>::value) wlp_store(Bs, b);
            else s3_store<LB::kc>(Bs, b);
        };
        // the prefetches are issued unconditionally (past kend the loaders read zeros or discarded
        // values without a branch), so every path through the loop has the same loads in flight and the
        // waits stay counted (s3_bload_chans)
        // (the A loads of a step are kept ahead of the B loads issued with it: the next step's operands
        // are then all but the newest 16 loads, a counted wait; reordered, the wait was vmcnt(0))
        if constexpr (!LA::pre) ldA(kbeg);   // (the weight planes were issued before the tables)
        __builtin_amdgcn_sched_barrier(0);
        lb.load(n0, kbeg, kend, vb);
        lb.load(n0, kbeg + kS3K, kend, vb1);
        for (int k0 = kbeg; k0 < kend; k0 += 2 * kS3K) {
            st(vb);
            __syncthreads();
            ldA(k0 + kS3K);
            __builtin_amdgcn_sched_barrier(0);
            lb.load(n0, k0 + 2 * kS3K, kend, vb);
            mma();
            __syncthreads();
            if (k0 + kS3K >= kend) break;
            st(vb1);
            __syncthreads();
            ldA(k0 + 2 * kS3K);
            __builtin_amdgcn_sched_barrier(0);
            lb.load(n0, k0 + 3 * kS3K, kend, vb1);
            mma();
            __syncthreads();
        }
    }
    const int64_t ldc = g.ldc ? g.ldc : g.N;
    // stacked classes (cls_wo == 0): output [split][cls][M][N]; else the parity scatter below
    const bool stacked = ncls > 1 && g.cls_wo == 0;
    float *C = g.C + (int64_t)(stacked ? kz * ncls + cls : kz) * g.M * ldc;
    const bool final_out = (int)gz == ncls;
    const float dv = (final_out && g.div) ? *g.div : 1.0f;
    if (ncls > 1 && !stacked) {
        // parity class: column n = source pixel (a, b) -> output pixel (2a + i, 2b + j)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int n = n0 + wn + 16 * b + jl;
            const int sa = n / g.cls_ws, sb = n - sa * g.cls_ws;
            const int64_t p = (int64_t)(2 * sa + (cls >> 1)) * g.cls_wo + 2 * sb + (cls & 1);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = m0 + wm + 16 * a + 4 * gk + r;
                    if (m < g.M && n < g.N) {
                        float v = acc[a][b][r];
                        if (final_out) {
                            if (g.bias) v = v + g.bias[m];
                            if (g.div) v = v / dv;
                            if (g.accum) v = C[(int64_t)m * ldc + p] + v;
                        }
                        C[(int64_t)m * ldc + p] = v;
                    }
                }
        }
        return;
    }
    if ((g.N & 3) != 0 || (reinterpret_cast<uintptr_t>(g.C) & 15) != 0) {
        // rows not float4-aligned (odd pixel counts): straight from the MFMA layout, 64-B runs
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
        return;
    }
    // float4-aligned rows: through LDS (the operand images are dead after the last barrier).
    // Each wave writes half of its 64 x 64 sub-tile at a time as [row][col] (row stride 68
    // floats) and reads it back as float4 runs, so 16 lanes store 256 contiguous bytes of a row
    float *E = reinterpret_cast<float *>(&ab) + wv * 32 * 68;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
        for (int a2 = 0; a2 < 2; ++a2)
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) E[(16 * a2 + 4 * gk + r) * 68 + 16 * b + jl] = acc[2 * hf + a2][b][r];
        __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): this wave's half-tile is in LDS (wave-local)
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int idx = lane + 64 * i, rr = idx >> 4, q = 4 * (idx & 15);
            const int m = m0 + wm + 32 * hf + rr, n = n0 + wn + q;
            if (m < g.M && n < g.N) {   // N % 4 == 0: a float4 run is all in or all out
                float4 v = *reinterpret_cast<const float4 *>(E + rr * 68 + q);
                float4 *c = reinterpret_cast<float4 *>(C + (int64_t)m * g.N + n);
                if (final_out) {
                    if (g.bias) {
                        const float bs = g.bias[m];
                        v.x = v.x + bs; v.y = v.y + bs; v.z = v.z + bs; v.w = v.w + bs;
                    }
                    if (g.div) { v.x = v.x / dv; v.y = v.y / dv; v.z = v.z / dv; v.w = v.w / dv; }
                    if (g.accum) {
                        const float4 o = *c;
                        v.x = o.x + v.x; v.y = o.y + v.y; v.z = o.z + v.z; v.w = o.w + v.w;
                    }
                }
                *c = v;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

template <class LA, class LB>
__global__ __launch_bounds__(256, 2) void k_gemm_s3(GemmArgs g, LA la, LB lb) {
    __shared__ __attribute__((aligned(16))) S3Smem sm;
    gemm_s3_body(g, la, lb, sm, blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z), gridDim.x, gridDim.y,
                 gridDim.z);
}

}  // namespace lrs

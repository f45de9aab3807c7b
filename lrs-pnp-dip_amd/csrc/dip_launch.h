// DIP low-rank prox, host side: conv geometry, tile and split-K choice, and the launchers of the
// kernels in dip_kernels.h / dip_bn.h / dip_sn.h / dip_train.h / dip_gemm.h / dip_pw.h / dip_wprep.h /
// dip_dgrad.h / dip_sm.h / dip_dir.h / dip_image.h (BatchNorm's form pickers and template dispatch are
// dip_bn.h's own).  No kernel is defined here.  Part of dipnet.hip's translation unit.
#pragma once
#include <math.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "dip_kernels.h"
#include "dip_bn.h"
#include "dip_sn.h"
#include "dip_train.h"
#include "dip_gemm.h"
#include "dip_pw.h"
#include "dip_wprep.h"
#include "dip_dgrad.h"
#include "dip_sm.h"
#include "dip_dir.h"
#include "dip_image.h"
#include "dip_up.h"
#include "ista_paths.h"

using namespace lrs;

namespace {

constexpr int kEw = 256;   // elementwise block size
constexpr int64_t kForkBigP = 9604;   // sigma beside the first conv: only where that conv's map is >= 98^2
// every BatchNorm of the engine: nn.BatchNorm2d's defaults
constexpr float kBnEps = 1e-5f, kBnMomentum = 0.1f;

inline unsigned ew_blocks(int64_t n, int64_t cap = 4096) {
    int64_t b = (n + kEw - 1) / kEw;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (unsigned)b;
}

// the defaults of a NULL lrs_dip_opts
inline lrs_dip_opts dip_opts(const lrs_dip_opts *o) {
    lrs_dip_opts d{};
    d.precision = LRS_DIP_SPLIT_BF16;
    d.upsample_dgrad = 0;
    return o ? *o : d;
}
inline bool dip_opts_ok(const lrs_dip_opts &o) {
    return (o.precision == LRS_DIP_F32 || o.precision == LRS_DIP_SPLIT_BF16) && (o.upsample_dgrad == 0 || o.upsample_dgrad == 1);
}

int make_geom(int Cin, int H, int W, int k, int stride, int pad, int pad_mode, int up, ConvGeom &g,
              const lrs_dip_opts *opts = nullptr) {
    const lrs_dip_opts o = dip_opts(opts);
    if (!dip_opts_ok(o)) return LRS_E_INVALID;
    if (Cin <= 0 || H <= 0 || W <= 0 || k <= 0 || stride <= 0 || pad < 0) return LRS_E_INVALID;
    if (pad_mode != LRS_PAD_ZERO && pad_mode != LRS_PAD_REFLECT) return LRS_E_INVALID;
    g.Cin = Cin; g.Hs = H; g.Ws = W;
    g.up = up ? 1 : 0; g.Hu = up ? 2 * H : H; g.Wu = up ? 2 * W : W;
    g.pad = pad; g.pad_mode = pad_mode; g.k = k; g.stride = stride;
    if (pad_mode == LRS_PAD_REFLECT && (pad >= g.Hu || pad >= g.Wu)) return LRS_E_INVALID;
    const int hp = g.Hu + 2 * pad, wp = g.Wu + 2 * pad;
    if (hp < k || wp < k) return LRS_E_INVALID;
    g.Ho = (hp - k) / stride + 1;
    g.Wo = (wp - k) / stride + 1;
    g.prec = o.precision;
    // Data gradient of an upsampled stride-1 conv (the U-Net's up_1..up_4: nearest x2, then 2 x 2 unpadded
    // or reflection-padded 3 x 3) as a stride-2 conv over dL/dz with a (k+1) x (k+1) effective kernel on
    // the source grid (dgrad_effective): 2.25x fewer products than correlating over the padded upsampled
    // domain and folding.  ke = k + 1, or 0 where the identity is not used; fixed with the geometry: the
    // workspace size, the weight-preparation table and the backward all read this one value.
    // Off by default: measured in the whole 196^2 training step (bench configs[2], 2 x 2 A/B runs) it is
    // ~1 % slower than the padded-domain correlation + fold -- the up_4 data-gradient work it saves ran
    // beside that layer's weight gradient anyway, and it adds a split-K reduce and the border launches
    // to the critical chain.  lrs_dip_opts::upsample_dgrad = 1 selects it (tests cover both).
    g.ke = 0;
    if (o.upsample_dgrad && g.up && g.stride == 1 && g.Hs >= 2 && g.Ws >= 2) {
        if (g.k == 3 && g.pad == 1) g.ke = 4;
        if (g.k == 2 && g.pad == 0) g.ke = 3;
    }
    return LRS_OK;
}

inline bool plain_unit(const ConvGeom &g) { return g.k == 1 && g.stride == 1 && g.pad == 0 && !g.up; }

struct Split { int S, kchunk; bool big; };   // big: 128x128 tiles (k_gemm) or 64x64 (k_gemm64)

constexpr int64_t kSplitMinTiles = 256;   // choose_split splits K below this many tiles
// ... into at most this many splits (a deep K: 256).  196^2 step, 2 rounds: 32 -> 1.327 ms, 64 -> 1.265,
// 128 -> 1.279, 256 -> 1.285; profiles/r04/split_cap/
constexpr int kSplitCap = 64;

// Tile choice and split-K: 128x128 tiles when they alone give >= 64 workgroups, else 64x64;
// then split K until ~512 workgroups (2 per CU), keeping >= 128 of K per split and <= 64 splits.
// (Measured with the f32 kernels: 128-tiles with deeper split-K on the small-N weight-gradient
// GEMMs, or a 1024-WG target, are slower at both the 36x36 and the 196x196 sizes.)
Split choose_split(int M, int N, int K, int precision = LRS_DIP_SPLIT_BF16, bool force_big = false, int target = 512) {
    const int64_t t128 = (int64_t)((M + kBM - 1) / kBM) * ((N + kBN - 1) / kBN);
    // long-K GEMMs (the weight gradients, K = pixels) take 128-tiles with deep split-K on the
    // split-bf16 path when that still gives >= 256 workgroups (measured 25-30 % faster at 196^2 and
    // 512^2; the 1x1 layer's 2-tile gradient is faster on 64-tiles)
    // Very long K with few tiles (a 1x1 conv's weight gradient over 512^2 pixels) splits up to 256
    // ways on the split-bf16 path, keeping >= 16 k-steps per workgroup.
    const bool deep = precision == LRS_DIP_SPLIT_BF16 && K >= 65536;
    const bool big = force_big || t128 >= 64 || (precision == LRS_DIP_SPLIT_BF16 && K >= 8192 && t128 >= 4) || deep;
    const int64_t tiles = big ? t128 : (int64_t)((M + kBM64 - 1) / kBM64) * ((N + kBN64 - 1) / kBN64);
    int S = 1;
    if (tiles < kSplitMinTiles) {
        S = (int)((target + tiles - 1) / tiles);   // ~2 workgroups per CU (256 and 1024 measured slower)
        const int smax = deep ? K / 512 : (K + 127) / 128;
        if (S > smax) S = smax;
        if (S > (deep ? 256 : kSplitCap)) S = deep ? 256 : kSplitCap;
        if (S < 1) S = 1;
    }
    const int bk = (big && precision == LRS_DIP_SPLIT_BF16) ? kBK32 : kBK;
    int kchunk = (int)round_up((K + S - 1) / S, bk);
    if (kchunk < bk) kchunk = bk;
    S = (K + kchunk - 1) / kchunk;
    if (S < 1) S = 1;
    return {S, kchunk, big};
}

// split-K scratch of an implicit-GEMM conv product (always 128-tiles, split-bf16)
int64_t s3_part_floats(int M, int N, int K) {
    const Split s = choose_split(M, N, K, LRS_DIP_SPLIT_BF16, true);
    return s.S > 1 ? (int64_t)s.S * M * N : 0;
}

int64_t gemm_part_floats(int M, int N, int K) {
    // sized for both precisions, so that the precision can change after a workspace was sized
    const Split a = choose_split(M, N, K, LRS_DIP_F32), b = choose_split(M, N, K, LRS_DIP_SPLIT_BF16);
    const int S = std::max(a.S, b.S);
    return S > 1 ? (int64_t)S * M * N : 0;
}

// the tail of a split-K product whose caller does not finish the sum itself: C (+)= sum of the partials
inline void split_reduce(const Split &s, const float *part, int M, int N, const float *bias, const float *div, int accum,
                         float *C, hipStream_t st) {
    if (s.S > 1)
        hipLaunchKernelGGL(k_gemm_reduce, dim3((unsigned)(((int64_t)M * N + kEw - 1) / kEw)), dim3(kEw), 0, st, part, s.S, M,
                           N, bias, div, accum, C);
}

// The tail every split-K product shares.  g holds the final output C; one split's partial is
// [g.M][pcols] floats (pcols = g.N, or the whole row where the kernel scatters parity classes).  In order:
// publish the split count; with more than one split (or to_part: a product whose own kernel sums its
// partials) check the scratch and send the output there; launch(g, grid) over tiles x (zmul * S); sum
// the partials into C (+ bias, / *div, accum) unless the caller finishes the sum (nsplit_out, to_part).
template <class Launch>
int split_launch(const Split &s, int64_t pcols, float *part, int64_t part_cap, GemmArgs g, dim3 tiles, int zmul,
                 int *nsplit_out, hipStream_t st, Launch launch, bool to_part = false) {
    if (nsplit_out) *nsplit_out = s.S;   // > 1: the caller finishes the split-K sum (no reduce here)
    float *C = g.C;
    if (s.S > 1 || to_part) {
        if (!part || part_cap < (int64_t)s.S * g.M * pcols) return LRS_E_WORKSPACE;
        g.C = part;
    }
    launch(g, dim3(tiles.x, tiles.y, (unsigned)(zmul * s.S)));
    if (!nsplit_out && !to_part) split_reduce(s, part, g.M, (int)pcols, g.bias, g.div, g.accum, C, st);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// C = op(A) op(B) (+ bias) (/ *div); part: split-K scratch (>= gemm_part_floats); prec: the
// conv's ConvGeom::prec
int gemm(int prec, int TA, int TB, const float *A, const float *B, float *C, const float *bias, const float *div, int M,
         int N, int K, float *part, int64_t part_cap, hipStream_t st, int accum = 0, int *nsplit_out = nullptr,
         bool force_big = false, int target = 512) {
    if (M <= 0 || N <= 0) return LRS_OK;
    const Split s = choose_split(M, N, K, prec, force_big, target);
    const int t = (TA ? 2 : 0) + (TB ? 1 : 0);   // the f32 kernels by (TA, TB)
    static void (*const k128[4])(GemmArgs) = {k_gemm<0, 0>, k_gemm<0, 1>, k_gemm<1, 0>, k_gemm<1, 1>};
    static void (*const k64[4])(GemmArgs) = {k_gemm64<0, 0>, k_gemm64<0, 1>, k_gemm64<1, 0>, k_gemm64<1, 1>};
    const dim3 tiles = s.big ? dim3((N + kBN - 1) / kBN, (M + kBM - 1) / kBM)
                             : dim3((N + kBN64 - 1) / kBN64, (M + kBM64 - 1) / kBM64);
    const auto launch = [&](const GemmArgs &g, dim3 grid) {
        if (s.big && prec == LRS_DIP_SPLIT_BF16) {
            const int lda = TA ? M : K, ldb = TB ? K : N;
#define LRS_S3(RA, RB)                                                                                        \
    hipLaunchKernelGGL((k_gemm_s3<LdDense<RA>, LdDense<RB>>), grid, dim3(kGemmThreads), 0, st, g, LdDense<RA>{A, lda, M}, \
                       LdDense<RB>{B, ldb, N})
            if (!TA && !TB) LRS_S3(true, false);
            else if (!TA && TB) LRS_S3(true, true);
            else if (TA && !TB) LRS_S3(false, false);
            else LRS_S3(false, true);
#undef LRS_S3
        } else {
            hipLaunchKernelGGL((s.big ? k128 : k64)[t], grid, dim3(kGemmThreads), 0, st, g);
        }
    };
    return split_launch(s, N, part, part_cap, GemmArgs{A, B, C, bias, div, M, N, K, s.kchunk, accum}, tiles, 1, nsplit_out,
                        st, launch);
}

inline int r16(int x) { return (x + 15) & ~15; }

// An upsampled, reflection-padded 3 x 3 stride-1 conv runs by output parity class in the network
// engine (dip_gemm.h LdUpFwdTM / LdUpDgradTM, 4/9 of the direct products); every other upsampled conv
// keeps the direct implicit GEMM over the upsampled grid.
inline bool upc_conv(const ConvGeom &g) {
    return g.up && g.k == 3 && g.pad == 1 && g.pad_mode == LRS_PAD_REFLECT && g.stride == 1 && g.Hs >= 2 && g.Ws >= 2;
}

// ---- small-map convs on k_conv_sm (dip_sm.h) ------------------------------------------------
// A split-bf16 conv runs there when it is not 1x1, k <= 3 and its output map is below kImplicitMinP
// (the maps that had the explicit im2col path).

// 64 x 64 tiles; split K so that the grid has ~kSmTargetWg workgroups (k per split a multiple of 64).
constexpr int64_t kSmTargetWg = 640;
Split sm_split(int M, int N, int K) {
    const int64_t T = (int64_t)((M + 63) / 64) * ((N + 63) / 64), W = kSmTargetWg;
    int64_t kc = round_up(std::max<int64_t>(1, ((int64_t)K * T + W - 1) / W), kSmK);
    if (kc > K) kc = round_up(K, kSmK);
    int S = (int)((K + kc - 1) / kc);
    kc = round_up((K + S - 1) / S, kSmK);
    S = (int)((K + kc - 1) / kc);
    return {S, (int)kc, false};
}

int64_t sm_part_floats(int M, int N, int K) {
    const Split s = sm_split(M, N, K);
    return s.S > 1 ? (int64_t)s.S * M * N : 0;
}

// C (+)= A B (+ bias) (/ *div) on k_conv_sm; split-K partials summed by k_gemm_reduce unless
// nsplit_out is given (the caller then finishes the sum, e.g. k_reduce_bn1); one_launch: no split
template <class LB, class LA = SmPre>
int sm_launch(const LA &la, const LB &lb, float *C, const float *bias, int M, int N, int K, int accum, float *part,
              int64_t part_cap, hipStream_t st, int *nsplit_out = nullptr, const float *div = nullptr,
              bool one_launch = false) {
    if (M <= 0 || N <= 0) return LRS_OK;
    Split s = sm_split(M, N, K);
    if (one_launch) s = {1, (int)round_up(K, kSmK), false};
    const GemmArgs a{nullptr, nullptr, C, bias, div, M, N, K, s.kchunk, accum};
    const auto launch = [&](const GemmArgs &g, dim3 grid) {
        hipLaunchKernelGGL((k_conv_sm<LB, LA>), grid, dim3(256), 0, st, g, la, lb);
    };
    return split_launch(s, N, part, part_cap, a, dim3((N + 63) / 64, (M + 63) / 64), 1, nsplit_out, st, launch);
}

// The weight-gradient gather table of a small-map conv: for tap t and output pixel p, the byte
// offset within a source channel plane of the value col[(c, t)][p] reads (kOob = zero pad); [kk][P]
std::vector<int> sm_wgrad_table(const ConvGeom &g) {
    const int kk = g.k * g.k, P = g.Ho * g.Wo;
    std::vector<int> t((size_t)kk * P, kOob);
    for (int kyx = 0; kyx < kk; ++kyx)
        for (int p = 0; p < P; ++p) {
            const int oy = p / g.Wo, ox = p - oy * g.Wo, ky = kyx / g.k, kx = kyx - ky * g.k;
            const int sy = conv_src(oy * g.stride + ky - g.pad, g.Hu, g.pad_mode, g.up);
            const int sx = conv_src(ox * g.stride + kx - g.pad, g.Wu, g.pad_mode, g.up);
            if (sy >= 0 && sx >= 0) t[(size_t)kyx * P + p] = 4 * (sy * g.Ws + sx);
        }
    return t;
}

// A small-map weight gradient on the side stream runs as one implicit k_conv_sm launch (no
// k_im2col, no split-K, no reduce) up to this many output pixels; above it the explicit col +
// split-K GEMM + reduce is faster (at 36^2: 18^2 maps 34 us one launch vs ~15 us for the three; the
// split-K implicit form 22 vs ~20 us).  196^2 step (13^2 maps, side stream) 1.275 -> 1.263 ms; on the
// single stream of a 36^2 net (no fork) 0.726 -> 0.735 ms, so it is used only where the net forks.
constexpr int kSmWgradOneLaunchP = 200;

// The conv's adjoint along one dimension: for tap t and source coordinate q, the output
// coordinates o with src(o, t) = q (reflection / zero pad, stride, x2 upsample), in increasing
// order, at most 2 (-1 = none).  False where some list would need more (the caller then keeps the
// explicit data gradient).
bool sm_adj_dim(int n_src, int n_up, int n_out, int k, int stride, int pad, int mode, int up, short *L) {
    for (int i = 0; i < k * n_src * 2; ++i) L[i] = -1;
    for (int o = 0; o < n_out; ++o)
        for (int t = 0; t < k; ++t) {
            const int q = conv_src(o * stride + t - pad, n_up, mode, up);
            if (q < 0) continue;
            short *e = L + (t * n_src + q) * 2;
            if (e[0] < 0) e[0] = (short)o;
            else if (e[1] < 0) e[1] = (short)o;
            else return false;
        }
    return true;
}

// The data-gradient gather table of a small-map conv: for tap (ty, tx) and input pixel q, the
// byte offsets (within a dL/dz plane) of the <= 2 x 2 output pixels that read q through it (the
// products of the per-dimension lists), kOob-padded; [kk][Q] int4.  Empty where sm_adj_dim fails.
std::vector<int> sm_adj_table(const ConvGeom &g) {
    std::vector<short> Ly((size_t)2 * g.k * g.Hs), Lx((size_t)2 * g.k * g.Ws);
    if (!sm_adj_dim(g.Hs, g.Hu, g.Ho, g.k, g.stride, g.pad, g.pad_mode, g.up, Ly.data()) ||
        !sm_adj_dim(g.Ws, g.Wu, g.Wo, g.k, g.stride, g.pad, g.pad_mode, g.up, Lx.data()))
        return {};
    const int Q = g.Hs * g.Ws;
    std::vector<int> t((size_t)4 * g.k * g.k * Q, kOob);
    for (int ty = 0; ty < g.k; ++ty)
        for (int tx = 0; tx < g.k; ++tx)
            for (int q = 0; q < Q; ++q) {
                const int qy = q / g.Ws, qx = q % g.Ws;
                int *e = t.data() + 4 * ((int64_t)(ty * g.k + tx) * Q + q);
                for (int a = 0; a < 2; ++a)
                    for (int b = 0; b < 2; ++b) {
                        const int oy = Ly[(ty * g.Hs + qy) * 2 + a], ox = Lx[(tx * g.Ws + qx) * 2 + b];
                        if (oy >= 0 && ox >= 0) e[2 * a + b] = 4 * (oy * g.Wo + ox);
                    }
            }
    return t;
}

int64_t conv_part_floats(const ConvGeom &g, int Cout) {
    const int P = g.Ho * g.Wo, kk = g.k * g.k, Kc = g.Cin * kk;
    int64_t m = gemm_part_floats(Cout, P, Kc);                       // forward
    const int64_t b = gemm_part_floats(Cout, Kc, P);                 // dW
    const int64_t c = gemm_part_floats(Kc, P, Cout);                 // dcol
    if (b > m) m = b;
    if (c > m) m = c;
    // implicit forms (tap-major K, channels rounded up to 16)
    m = std::max(m, std::max(s3_part_floats(Cout, P, kk * r16(g.Cin)), s3_part_floats(Cout, Kc, P)));
    const int Qp = (g.Hu + 2 * g.pad) * (g.Wu + 2 * g.pad);
    m = std::max(m, s3_part_floats(g.Cin, Qp, kk * r16(Cout)));
    if (const int ke = g.ke) m = std::max(m, s3_part_floats(g.Cin, g.Hs * g.Ws, ke * ke * r16(Cout)));
    m = std::max(m, std::max(sm_part_floats(Cout, P, kk * r16(g.Cin)), sm_part_floats(g.Cin, g.Hs * g.Ws, kk * r16(Cout))));
    m = std::max(m, sm_part_floats(Cout, Kc, P));   // the small-map weight gradient (SmWgrad)
    return m;
}

// split-K scratch of a parity-class conv (network engine only): forward partials over the whole
// output, the data gradient over the extended source grid, the weight gradient [split][cls][Cout][4 Cin]
int64_t upc_part_floats(const ConvGeom &g, int Cout) {
    const int64_t P = (int64_t)g.Ho * g.Wo;
    int64_t m = 0;
    const Split f = choose_split(Cout, 4 * g.Hs * g.Ws, 4 * r16(g.Cin), LRS_DIP_SPLIT_BF16, true);
    if (f.S > 1) m = (int64_t)f.S * Cout * P;
    m = std::max(m, s3_part_floats(g.Cin, (g.Hs + 2) * (g.Ws + 2), 16 * r16(Cout)));
    const Split w = choose_split(Cout, 16 * g.Cin, g.Hs * g.Ws, LRS_DIP_SPLIT_BF16, true);
    return std::max(m, (int64_t)w.S * 16 * Cout * g.Cin);
}

// bf16 elements of a conv's pre-split weight planes (dip_wprep.h): the forward operand's three planes
// first -- WF [3][Cout][kk Cp], or by parity class (upc) WUF [3][4][Cout][4 Cp] -- then the data-gradient
// operand's: WD [3][Cin][kk Cop], WE [3][Cin][ke^2 Cop] with an effective kernel, or WUD [3][Cin][16 Cop]
struct WprepElems {
    int64_t fwd, dgrad;
    int64_t total() const { return fwd + dgrad; }
};
inline WprepElems wprep_elems(const ConvGeom &g, int Cout, bool upc) {
    const int kk = g.k * g.k, taps_d = upc ? 16 : g.ke ? g.ke * g.ke : kk;
    return {3 * (int64_t)Cout * (upc ? 16 : kk) * r16(g.Cin), 3 * (int64_t)g.Cin * taps_d * r16(Cout)};
}

// split-K workgroup target of a forward conv whose partials a fused BN kernel finishes: fewer
// splits than the GEMMs' 512 (the BN kernel, one workgroup per channel, re-reads every partial):
// 196^2 step 1.336 -> 1.312 ms at 384 (A/B on one box: 256 1.317, 320 1.313).  The workspace is
// sized for 512, so a larger target fails with LRS_E_WORKSPACE.
constexpr int kFwdSplitWg = 384;

// Split target of the padded-domain data-gradient GEMMs whose split-K partials k_fold_pad sums
// (every partial is re-read by the fold, as by the forward BN kernels above); at most the 512 the
// workspace is sized for.
constexpr int kDgradSplitWg = 512;

// Implicit-GEMM conv product on the split-bf16 kernel (always 128-tiles), with gemm()'s split-K tail.
template <class LA, class LB>
int gemm_s3_conv(const LA &la, const LB &lb, float *C, const float *bias, const float *div, int M, int N, int K,
                 float *part, int64_t part_cap, hipStream_t st, int *nsplit_out = nullptr, int accum = 0,
                 int target = 512) {
    if (M <= 0 || N <= 0) return LRS_OK;
    const Split s = choose_split(M, N, K, LRS_DIP_SPLIT_BF16, true, target);
    const GemmArgs a{nullptr, nullptr, C, bias, div, M, N, K, s.kchunk, accum};
    const auto launch = [&](const GemmArgs &g, dim3 grid) {
        hipLaunchKernelGGL((k_gemm_s3<LA, LB>), grid, dim3(kGemmThreads), 0, st, g, la, lb);
    };
    return split_launch(s, N, part, part_cap, a, dim3((N + 127) / 128, (M + 127) / 128), 1, nsplit_out, st, launch);
}

// Forward of an upsampled 3 x 3 conv by output parity class: one launch, gridDim.z = 4 classes x
// split-K; y (or the split-K partials) over the whole output.  wpre = the WUF planes.
int upc_fwd(const ConvGeom &g, const float *x, const __bf16 *wpre, const float *bias, int Cout, float *y, float *part,
            int64_t part_cap, hipStream_t st, int *nsplit_out) {
    const int Cp = r16(g.Cin), Q = g.Hs * g.Ws, K = 4 * Cp;
    const int64_t P = (int64_t)g.Ho * g.Wo;
    const Split s = choose_split(Cout, 4 * Q, K, LRS_DIP_SPLIT_BF16, true, nsplit_out ? kFwdSplitWg : 512);
    const GemmArgs a{nullptr, nullptr, y, bias, nullptr, Cout, Q, K, s.kchunk, 0, 4, g.Ws, g.Wo, P};
    const auto launch = [&](const GemmArgs &ga, dim3 grid) {
        hipLaunchKernelGGL((k_gemm_s3<LdPre, LdUpFwdTM>), grid, dim3(kGemmThreads), 0, st, ga,
                           LdPre{wpre, (int64_t)4 * Cout * K, K, Cout, (int64_t)Cout * K},
                           LdUpFwdTM{x, g.Cin * Q * 4, g, Cp, nullptr});
    };
    return split_launch(s, P, part, part_cap, a, dim3((Q + 127) / 128, (Cout + 127) / 128), 4, nsplit_out, st, launch);
}

// Its data gradient: gxe over the source grid extended by one pixel (one GEMM with K = 4 classes x
// 4 effective taps x Cout, into the scratch gxe), then k_fold_pad in kPadClamp mode adds the outside
// ring onto the border pixels (gx += when accum).  wd = the WUD planes.
int upc_dgrad(const ConvGeom &g, const float *gz, const __bf16 *wd, int Cout, float *gx, float *gxe, float *part,
              int64_t part_cap, hipStream_t st, int accum) {
    const int Cop = r16(Cout), K = 16 * Cop, Qe = (g.Hs + 2) * (g.Ws + 2);
    int nsplit = 1;   // split-K partials are summed inside the fold
    int rc = gemm_s3_conv(LdPre{wd, (int64_t)g.Cin * K, K, g.Cin}, LdUpDgradTM{gz, Cout * g.Ho * g.Wo * 4, g, Cout, Cop, nullptr},
                          gxe, nullptr, nullptr, g.Cin, Qe, K, part, part_cap, st, &nsplit, 0,
                          kDgradSplitWg);
    if (rc) return rc;
    ConvGeom fg = g;
    fg.up = 0;
    fg.Hu = g.Hs;
    fg.Wu = g.Ws;
    fg.pad = 1;
    fg.pad_mode = kPadClamp;
    const dim3 grid((unsigned)((g.Hs * g.Ws + 255) / 256), (unsigned)std::min(g.Cin, 65535));
    hipLaunchKernelGGL(k_fold_pad, grid, dim3(256), 0, st, nsplit > 1 ? part : gxe, nsplit, (int64_t)g.Cin * Qe, fg, gx,
                       accum);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// Its weight gradient: per class dWE_cls = dL/dz(class pixels) x col_cls^T (one launch, classes and
// split-K over gridDim.z, partials [split][cls][Cout][4 Cin] in part), then k_upc_wgrad_combine sums
// splits and classes into dW (/ *div).
int upc_wgrad(const ConvGeom &g, const float *gz, const float *x, const float *div, int Cout, float *gw, float *part,
              int64_t part_cap, hipStream_t st, int target = 512) {
    const int Q = g.Hs * g.Ws, N = 4 * g.Cin;
    const Split s = choose_split(Cout, 4 * N, Q, LRS_DIP_SPLIT_BF16, true, target);
    const GemmArgs a{nullptr, nullptr, part, nullptr, nullptr, Cout, N, Q, s.kchunk, 0, 4, g.Ws, 0, 0};
    const auto launch = [&](const GemmArgs &ga, dim3 grid) {
        hipLaunchKernelGGL((k_gemm_s3<LdGzCls, LdWgradCls>), grid, dim3(kGemmThreads), 0, st, ga,
                           LdGzCls{gz, g.Hs, g.Ws, g.Wo, Cout, 0}, LdWgradCls{x, g.Cin * Q * 4, g, nullptr, 0, 0});
    };
    // to_part: the partials go to the scratch with one split too (k_upc_wgrad_combine sums the classes)
    const int rc = split_launch(s, 4 * N, part, part_cap, a, dim3((N + 127) / 128, (Cout + 127) / 128), 4, nullptr, st, launch,
                                true);
    if (rc) return rc;
    const int64_t n = (int64_t)Cout * g.Cin * 9;
    hipLaunchKernelGGL(k_upc_wgrad_combine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, s.S, Cout, g.Cin,
                       div, gw);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// implicit GEMM: k <= 3 (LDS tables) and both operand tensors addressable by 32-bit buffer offsets
inline bool conv_implicit_ok(const ConvGeom &g, int Cout) {
    return g.k <= 3 && (int64_t)g.Cin * g.Hs * g.Ws * 4 < kOob && (int64_t)Cout * g.Ho * g.Wo * 4 < kOob;
}

// The engine runs a conv as an implicit GEMM from this many output pixels up; below it the maps
// are small enough that an explicit im2col into a cached col buffer plus the 64-tile GEMMs is
// faster (round 1, at 36x36: 1.23 vs 1.41 ms per U-Net step).  Round 4 re-measured the kernels of
// today: 2048 -> 1024 moves the 36^2 maps (1296 pixels) to the implicit paths, 36^2 step 0.652 ->
// 0.638 ms, and the skip net's 32^2 maps, 512^2 step 9.27 -> 9.23 ms; 512 (the 196^2 net's 25^2 maps
// too) is slower there, 1.244 -> 1.288 ms (profiles/r04/implicit_min_p/).
constexpr int64_t kImplicitMinP = 1024;

// split w into the bf16 planes of the forward operand (and of the data-gradient one if wd)
int wprep(const ConvGeom &g, const float *w, int Cout, __bf16 *wf, __bf16 *wd, hipStream_t st) {
    const int kk = g.k * g.k;
    const int64_t elems = wprep_elems(g, Cout, false).total();
    if (elems >= INT32_MAX / 3) return LRS_E_UNSUPPORTED;   // k_conv_prep's 32-bit indices
    const int64_t n = elems / 3;
    const ConvPrep c{w, nullptr, wf, wd, Cout, g.Cin, kk, r16(g.Cin), r16(Cout), -1, g.k, wd ? g.ke : 0};
    hipLaunchKernelGGL(k_conv_prep1, dim3(ew_blocks(n, 2048)), dim3(256), 0, st, c);
    return LRS_OK;
}

// k_pw instantiations: MT row blocks x NB 16-pixel column blocks, and the workgroups per CU their
// registers allow (one wave per SIMD each; gfx950: 512 VGPRs per SIMD lane over the waves, in
// granules of 8; the counts of the current build: 80, 150, 192, 234, 198).  48-pixel workgroups
// (NB = 3) for the LDS-bound K = 198 data gradient measured ~10 us per 196^2 step slower (A/B)
// and were dropped.
struct PwKernel {
    int mt, nb, wg_per_cu;
    void (*fn)(PwArgs);
};
static const PwKernel kPwKernels[] = {
    {1, 4, 6, k_pw<1, 4>}, {2, 4, 3, k_pw<2, 4>}, {3, 4, 2, k_pw<3, 4>}, {4, 4, 2, k_pw<4, 4>}, {4, 5, 2, k_pw<4, 5>},
};

// Pointwise conv product on k_pw (A: pre-split planes [3][M][lda], B: [K][N] fp32).
// The pixel width of a workgroup is chosen per launch: the fewest rounds of the CU slots (LDS
// 3 x 16 NB x ldsrow bytes and the registers both limit them) times the per-workgroup work (NB),
// wider on ties.  At 196^2 the 198-row last 1x1 runs on 80 pixels: 481 workgroups, one round of
// 2 per CU instead of 1.2 rounds at 64 (A/B: -10 us per step).
struct PwHead {   // the fused masked-MSE head of a network's last conv (PwArgs::tgt)
    const float *tgt, *msk;
    int64_t mstride;   // mask row stride: 0 ([P], every channel) or P ([C][P])
    float *gz;
    double *hpart;
    float norm;
    int *nwg_out;   // the grid the launch used (k_head_reduce's partial count)
};

int pw_launch(const __bf16 *A, int64_t pstride, int lda, int M, const float *B, int K, int64_t N, float *C,
              const float *bias, int accum, hipStream_t st, int act = 0, const PwHead *head = nullptr) {
    if (M <= 0 || N <= 0) return LRS_OK;
    if (M > 256 || lda < K || lda % 16) return LRS_E_UNSUPPORTED;
    const int Kp32 = (int)round_up(lda, 32), ldsrow = pw_ldsrow(Kp32);
    static std::atomic<uint64_t> attr_set[sizeof(kPwKernels) / sizeof(kPwKernels[0])];   // per device
    for (size_t i = 0; i < sizeof(kPwKernels) / sizeof(kPwKernels[0]); ++i)   // up to K = 256: 3 x 80 x 528 B
        if (const int rc = lds_opt_in((const void *)kPwKernels[i].fn, 3 * 80 * pw_ldsrow(256), attr_set[i])) return rc;
    if (Kp32 > 256 || (int64_t)K * N * 4 >= kOob || 3 * pstride * 2 >= kOob) return LRS_E_UNSUPPORTED;
    const PwArgs a{A, pstride, lda, B, K, N, C, bias, M, Kp32, ldsrow, accum, act};
    const int mt = (M + 63) / 64;
    const PwKernel *best = nullptr;
    int64_t best_cost = 0;
    for (const PwKernel &k : kPwKernels) {
        if (k.mt != mt) continue;
        const int lds = 3 * 16 * k.nb * ldsrow;
        const int per_cu = std::min(k.wg_per_cu, (160 * 1024) / lds);
        const int64_t wgs = (N + 16 * k.nb - 1) / (16 * k.nb);
        const int64_t rounds = (wgs + 256 * per_cu - 1) / (256 * per_cu);
        const int64_t cost = rounds * k.nb;
        if (!best || cost < best_cost || (cost == best_cost && k.nb > best->nb)) {
            best = &k;
            best_cost = cost;
        }
    }
    if (!best) return LRS_E_UNSUPPORTED;
    const int npx = 16 * best->nb;
    PwArgs ah = a;
    if (head) {
        ah.tgt = head->tgt;
        ah.msk = head->msk;
        ah.mstride = head->msk ? head->mstride : 0;
        ah.gz = head->gz;
        ah.hpart = head->hpart;
        ah.hnorm = head->norm;
        *head->nwg_out = (int)((N + npx - 1) / npx);
    }
    hipLaunchKernelGGL(best->fn, dim3((unsigned)((N + npx - 1) / npx)), dim3(256), 3 * npx * ldsrow, st, ah);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

inline bool pw_ok(const ConvGeom &g, int Cout) { return plain_unit(g) && Cout <= 256 && r16(g.Cin) <= 256 && r16(Cout) <= 256; }

// y = conv(x) + bias.  Explicit (col != NULL): im2col + GEMM.  Implicit (col == NULL, wpre =
// the weight planes from wprep): tap-major implicit GEMM.
// act_pw: activation for the pointwise kernel's epilogue (a 1x1 conv without BN), applied only there.
int conv_fwd(const ConvGeom &g, const float *x, const float *w, const float *bias, int Cout, float *col, float *y,
             float *part, int64_t part_cap, hipStream_t st, const __bf16 *wpre = nullptr, int *nsplit_out = nullptr,
             int act_pw = 0, const PwHead *head = nullptr) {
    const int P = g.Ho * g.Wo, Kc = g.Cin * g.k * g.k;
    if (nsplit_out) *nsplit_out = 1;
    const float *B = x;
    if (plain_unit(g) && wpre)      // 1x1: pointwise kernel on the pre-split weights
        return pw_launch(wpre, (int64_t)Cout * r16(g.Cin), r16(g.Cin), Cout, x, g.Cin, P, y, bias, 0, st, act_pw, head);
    if (head) return LRS_E_UNSUPPORTED;
    if (!plain_unit(g) && !col) {   // implicit im2col
        if (!conv_implicit_ok(g, Cout) || !wpre) return LRS_E_UNSUPPORTED;
        const int kk = g.k * g.k, Cp = r16(g.Cin);
        return gemm_s3_conv(LdPre{wpre, (int64_t)Cout * kk * Cp, kk * Cp, Cout},
                            LdFwdTM{x, g.Cin * g.Hs * g.Ws * 4, g, Cp, nullptr}, y, bias, nullptr, Cout, P, kk * Cp,
                            part, part_cap, st, nsplit_out, 0, nsplit_out ? kFwdSplitWg : 512);
    }
    if (!plain_unit(g)) {
        const dim3 grid((unsigned)((P + 255) / 256), (unsigned)std::min(Kc, 65535));
        hipLaunchKernelGGL(k_im2col, grid, dim3(256), 0, st, x, g, col);
        B = col;
    }
    return gemm(g.prec, 0, 0, w, B, y, bias, nullptr, Cout, P, Kc, part, part_cap, st, 0, nsplit_out);
}

// gw = gz col^T / *div.  implicit (a conv that is not 1x1): `col` is the conv input x and col^T is gathered
// inside the GEMM.  wsplit_out: the caller finishes the split-K sum (k_adam's AdamPend).
int conv_wgrad(const ConvGeom &g, const float *gz, const float *col, const float *div, int Cout, float *gw, float *part,
               int64_t part_cap, hipStream_t st, bool implicit, int *wsplit_out = nullptr, int wtarget = 512) {
    const int P = g.Ho * g.Wo, Kc = g.Cin * g.k * g.k;
    if (implicit && !plain_unit(g)) {
        if (!conv_implicit_ok(g, Cout)) return LRS_E_UNSUPPORTED;
        return gemm_s3_conv(LdDense<true>{gz, P, Cout}, LdWgradTM{col, g.Cin * g.Hs * g.Ws * 4, g, nullptr, 0}, gw,
                            nullptr, div, Cout, Kc, P, part, part_cap, st, wsplit_out, 0, wtarget);
    }
    // a 1x1 conv's weight gradient (K = all pixels): 128-tiles with deep split-K on the split-bf16
    // kernel (A/B in the 196^2 training step, configs[2]: 5.50 -> 5.65 outer it/s against the f32
    // 64-tile kernel; alone the two are within 12 %, but the f32 kernel's 512 workgroups hold the
    // CUs the concurrent data-gradient chain needs for longer)
    return gemm(g.prec, 0, 1, gz, col, gw, nullptr, div, Cout, Kc, P, part, part_cap, st, 0, wsplit_out, plain_unit(g),
                wtarget);
}

// ---- the four forms of a conv's data gradient gx (+)= conv^T(dL/dz); conv_dgrad picks one ----------

// 1x1: k_pw on the W^T planes (wprep's WD) where the conv has planes, else the dense GEMM W^T gz
int dgrad_pointwise(const ConvGeom &g, const float *gz, const float *w, const __bf16 *wpre, int Cout, float *gx,
                    float *part, int64_t part_cap, hipStream_t st, int accum) {
    const int P = g.Ho * g.Wo;
    if (wpre)
        return pw_launch(wpre + wprep_elems(g, Cout, false).fwd, (int64_t)g.Cin * r16(Cout), r16(Cout), g.Cin, gz, Cout, P,
                         gx, nullptr, accum, st);
    return gemm(g.prec, 1, 0, w, gz, gx, nullptr, nullptr, g.Cin, P, Cout, part, part_cap, st, accum);
}

// An upsampled stride-1 conv with an effective kernel (ConvGeom::ke): gx = the stride-2 (ke x ke, zero
// pad 1) conv of dL/dz with the effective weights we (k_conv_prep's WE), then the reflection terms of
// the border rows / columns (dip_dgrad.h k_up_border_*; border: their scratch S and corr)
int dgrad_effective(const ConvGeom &g, const float *gz, const float *w, const __bf16 *we, int Cout, float *gx,
                    float *border, float *part, int64_t part_cap, hipStream_t st) {
    const int P = g.Ho * g.Wo, ke = g.ke, Cop = r16(Cout), ke2 = ke * ke;
    ConvGeom ge{};
    ge.Cin = Cout; ge.Hs = g.Ho; ge.Ws = g.Wo; ge.up = 0; ge.Hu = g.Ho; ge.Wu = g.Wo;
    ge.pad = 1; ge.pad_mode = LRS_PAD_ZERO; ge.k = ke; ge.stride = 2; ge.Ho = g.Hs; ge.Wo = g.Ws;
    if ((g.Ho + 2 - ke) / 2 + 1 != g.Hs || (g.Wo + 2 - ke) / 2 + 1 != g.Ws) return LRS_E_INVALID;
    const int rc = gemm_s3_conv(LdPre{we, (int64_t)g.Cin * ke2 * Cop, ke2 * Cop, g.Cin},
                                LdFwdTM{gz, Cout * P * 4, ge, Cop, nullptr}, gx, nullptr, nullptr, g.Cin, g.Hs * g.Ws,
                                ke2 * Cop, part, part_cap, st);
    if (rc) return rc;
    if (g.pad_mode == LRS_PAD_REFLECT && g.k == 3) {
        const int Lmax = std::max(g.Ws, g.Hs);
        float *S = border, *corr = border + (int64_t)4 * 3 * Cout * Lmax;
        hipLaunchKernelGGL(k_up_border_s, dim3((unsigned)((12 * Lmax + 255) / 256), (unsigned)Cout), dim3(256), 0, st,
                           gz, Cout, g.Hs, g.Ws, Lmax, S);
        hipLaunchKernelGGL(k_up_border_mm, dim3(4, (unsigned)((g.Cin + kUbC - 1) / kUbC), (unsigned)((Lmax + 127) / 128)),
                           dim3(256), 0, st, S, w, g.Cin, Cout, g.Hs, g.Ws, Lmax, corr);
        const int nper = 2 * g.Ws + 2 * (g.Hs - 2);
        hipLaunchKernelGGL(k_up_border_add, dim3((unsigned)((nper + 255) / 256), (unsigned)g.Cin), dim3(256), 0, st,
                           corr, g.Cin, g.Hs, g.Ws, Lmax, gx);
    }
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// Stride 1: gxp = W^T (x) gz over the padded, upsampled domain (implicit GEMM on the WD planes wd, into
// dcol), then the fold of the padding / upsample, which also sums the split-K partials
int dgrad_padded(const ConvGeom &g, const float *gz, const __bf16 *wd, int Cout, float *gx, float *dcol, float *part,
                 int64_t part_cap, hipStream_t st, int accum) {
    const int P = g.Ho * g.Wo, kk = g.k * g.k, Cop = r16(Cout), Qp = (g.Hu + 2 * g.pad) * (g.Wu + 2 * g.pad);
    int nsplit = 1;
    const int rc = gemm_s3_conv(LdPre{wd, (int64_t)g.Cin * kk * Cop, kk * Cop, g.Cin},
                                LdDgradTM{gz, Cout * P * 4, g, Cout, Cop, nullptr}, dcol, nullptr, nullptr, g.Cin, Qp,
                                kk * Cop, part, part_cap, st, &nsplit, 0, kDgradSplitWg);
    if (rc) return rc;
    if (nsplit == 1 && !g.up && g.Ws % 4 == 0 && g.Cin <= 65535 && ((uintptr_t)gx & 15) == 0) {   // one partial: row quads
        const int q = g.Hs * (g.Ws / 4);
        hipLaunchKernelGGL(k_fold_pad1q, dim3((unsigned)((q + 255) / 256), (unsigned)g.Cin), dim3(256), 0, st, dcol,
                           g, gx, accum);
    } else {
        const dim3 grid((unsigned)((g.Hs * g.Ws + 255) / 256), (unsigned)std::min(g.Cin, 65535));
        hipLaunchKernelGGL(k_fold_pad, grid, dim3(256), 0, st, nsplit > 1 ? part : dcol, nsplit, (int64_t)g.Cin * Qp,
                           g, gx, accum);
    }
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// Any geometry: dcol = W^T gz (explicit, Kc x P floats), then col2im
int dgrad_col2im(const ConvGeom &g, const float *gz, const float *w, int Cout, float *gx, float *dcol, float *part,
                 int64_t part_cap, hipStream_t st, int accum) {
    const int P = g.Ho * g.Wo, Kc = g.Cin * g.k * g.k;
    const int rc = gemm(g.prec, 1, 0, w, gz, dcol, nullptr, nullptr, Kc, P, Cout, part, part_cap, st);
    if (rc) return rc;
    const dim3 grid((unsigned)((g.Hs * g.Ws + 255) / 256), (unsigned)std::min(g.Cin, 65535));
    if (g.stride == 1) hipLaunchKernelGGL(k_col2im<1>, grid, dim3(256), 0, st, dcol, g, gx, accum);
    else if (g.stride == 2) hipLaunchKernelGGL(k_col2im<2>, grid, dim3(256), 0, st, dcol, g, gx, accum);
    else hipLaunchKernelGGL(k_col2im<0>, grid, dim3(256), 0, st, dcol, g, gx, accum);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// gx (+)= col2im(w^T gz).  dcol: Kc * P floats when the conv is not 1x1 (NULL: only the forms without it).
// implicit with wpre (the weight planes from wprep / k_conv_prep): the data gradient reads the planes
// after the forward operand's (WD, or WE with an effective kernel).
int conv_dgrad(const ConvGeom &g, const float *gz, const float *w, int Cout, float *gx, float *dcol, float *part,
               int64_t part_cap, hipStream_t st, int accum, bool implicit, const __bf16 *wpre) {
    if (plain_unit(g)) return dgrad_pointwise(g, gz, w, wpre, Cout, gx, part, part_cap, st, accum);
    const __bf16 *wd = (implicit && wpre) ? wpre + wprep_elems(g, Cout, false).fwd : nullptr;
    const int P = g.Ho * g.Wo, Kc = g.Cin * g.k * g.k;
    const bool refl_border = g.pad_mode == LRS_PAD_REFLECT && g.k == 3;
    // the border scratch (S and corr) lives in the col-gradient buffer, unused on that path
    const bool border_fits = dcol && (int64_t)4 * (3 * Cout + g.Cin) * std::max(g.Ws, g.Hs) <= (int64_t)Kc * P;
    if (wd && g.ke && !accum && (!refl_border || border_fits))
        return dgrad_effective(g, gz, w, wd, Cout, gx, dcol, part, part_cap, st);
    if (!dcol) return LRS_E_WORKSPACE;
    const int Qp = (g.Hu + 2 * g.pad) * (g.Wu + 2 * g.pad);
    if (wd && g.stride == 1 && (int64_t)g.Cin * Qp <= (int64_t)Kc * P)
        return dgrad_padded(g, gz, wd, Cout, gx, dcol, part, part_cap, st, accum);
    return dgrad_col2im(g, gz, w, Cout, gx, dcol, part, part_cap, st, accum);
}

inline bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// BatchNorm (+ activation) of z as stored, forward and backward: the form from dip_bn.h's pickers
// (register resident, one workgroup per channel, or the S-way split; without gamma the activation alone)
int bn_fwd(const float *z, float *y, const float *gamma, const float *beta, float *mean, float *invstd, float *rm,
           float *rv, int C, int64_t P, int act, float eps, float mom, double *part, hipStream_t st, int lip = 1) {
    const int S = bn_split(P);
    const int vec = (P % 4 == 0 && al16(z) && al16(y)) ? 1 : 0;
    int chunk = (int)((P + S - 1) / S);
    if (vec) chunk = (chunk + 3) & ~3;
    BnArgs a{z, y, gamma, beta, mean, invstd, rm, rv, part, C, (int)P, S, chunk, gamma ? 1 : 0, act, eps, mom, lip,
             vec};
    if (const int nq = gamma ? bn_reg_q(P, vec) : 0) {
        launch_bn_fwd_r(nq, nullptr, 0, nullptr, a, nullptr, st);
    } else if (gamma && bn_one_wg(P)) {
        hipLaunchKernelGGL(k_bn_fwd1, dim3(1, C), dim3(bn1_threads(P)), 0, st, a);
    } else {
        if (gamma) hipLaunchKernelGGL(k_bn_stats, dim3(S, C), dim3(kBnThreads), 0, st, a);
        hipLaunchKernelGGL(k_bn_apply, dim3(S, C), dim3(kBnThreads), 0, st, a);
    }
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

int bn_bwd(const float *gy, const float *y, const float *z, const float *gamma, const float *mean,
           const float *invstd, float *gz, float *ggamma, float *gbeta, float *gbias, int C, int64_t P, int act,
           double *part, hipStream_t st, int lip = 1, int accum = 0, const float *beta = nullptr) {
    const int S = bn_split(P);
    const int vec = (P % 4 == 0 && al16(gy) && al16(y) && al16(z) && al16(gz)) ? 1 : 0;
    int chunk = (int)((P + S - 1) / S);
    if (vec) chunk = (chunk + 3) & ~3;
    BnBwdArgs a{gy, y, z, gamma, mean, invstd, gz, ggamma, gbeta, gbias, part, C, (int)P, S, chunk,
                gamma ? 1 : 0, act, lip, accum, vec, gamma ? beta : nullptr};
    if (const int nq = gamma ? bn_reg_q(P, vec) : 0) {
        launch_bn_bwd_r(nq, a, st);
    } else if ((gamma || gbias) && bn_one_wg(P)) {
        hipLaunchKernelGGL(k_bn_bwd1, dim3(1, C), dim3(bn1_threads(P)), 0, st, a);
    } else {
        if (gamma || gbias) hipLaunchKernelGGL(k_bn_bwd_stats, dim3(S, C), dim3(kBnThreads), 0, st, a);
        hipLaunchKernelGGL(k_bn_bwd_apply, dim3(S, C), dim3(kBnThreads), 0, st, a);
    }
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// ---- the Deep Decoder stage's kernels (dip_up.h) -------------------------------------------------
inline bool dec_act_ok(int act) { return act == LRS_ACT_NONE || act == LRS_ACT_LRELU || act == LRS_ACT_RELU; }

// Block (bx, 256 / bx) over (source column pairs, source rows): bx = the width of 16, 32 or 64 that pads
// the row of column pairs least (the wider on ties); grid z = channels.
struct Up2Grid { dim3 grid, block; };
inline int up2_grid(int C, int H, int W, Up2Grid &u) {
    if (C <= 0 || H <= 0 || W <= 0) return LRS_E_INVALID;
    if (C > 65535 || (int64_t)4 * H * W > INT32_MAX) return LRS_E_UNSUPPORTED;
    const int wp = (W + 1) / 2;
    int bx = 64;
    for (int b : {32, 16})
        if ((wp + b - 1) / b * b < (wp + bx - 1) / bx * bx) bx = b;
    const int by = 256 / bx;
    if ((H + by - 1) / by > 65535) return LRS_E_UNSUPPORTED;
    u.block = dim3(bx, by);
    u.grid = dim3((wp + bx - 1) / bx, (H + by - 1) / by, C);
    return LRS_OK;
}

// a[C][2H][2W] = act(up2(z[C][H][W]))
int up2_fwd(const float *z, int C, int H, int W, int act, float *a, hipStream_t st) {
    Up2Grid u;
    if (const int rc = up2_grid(C, H, W, u)) return rc;
    const int vec = (W % 2 == 0 && al16(a)) ? 1 : 0;
    hipLaunchKernelGGL(k_up2_bilinear_act, u.grid, u.block, 0, st, z, a, H, W, act, vec);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// gz[C][H][W] = up2^T(ga .* act'(a))
int up2_bwd(const float *ga, const float *a, int C, int H, int W, int act, float *gz, hipStream_t st) {
    Up2Grid u;
    if (const int rc = up2_grid(C, H, W, u)) return rc;
    const int vec = (W % 2 == 0 && al16(ga) && al16(a)) ? 1 : 0;
    hipLaunchKernelGGL(k_up2_bilinear_act_bwd, u.grid, u.block, 0, st, ga, a, gz, H, W, act, vec);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// the stage that does not upsample: a = act(z) / gz = ga .* act'(a) over n elements
int dec_act_fwd_launch(const float *z, float *a, int64_t n, int act, hipStream_t st) {
    const int vec = (al16(z) && al16(a)) ? 1 : 0;
    hipLaunchKernelGGL(k_dec_act, dim3(ew_blocks((n + 3) / 4)), dim3(kEw), 0, st, z, a, n, act, vec);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}
int dec_act_bwd_launch(const float *ga, const float *a, float *gz, int64_t n, int act, hipStream_t st) {
    const int vec = (al16(ga) && al16(a) && al16(gz)) ? 1 : 0;
    hipLaunchKernelGGL(k_dec_act_bwd, dim3(ew_blocks((n + 3) / 4)), dim3(kEw), 0, st, ga, a, gz, n, act, vec);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// One launch: direct fp32 conv + BatchNorm (+ act), one workgroup per output channel (k_conv_bn_dir,
// dip_dir.h); dg from dir_geom(g).  The caller checks the launch.
void dir_launch(const ConvGeom &g, const DirGeom &dg, const float *x, const float *w, const float *bias, const BnArgs &a,
                hipStream_t st) {
    const dim3 grid(1, a.C);
#define LRS_DIR(KS, S)                                                                                         \
    do {                                                                                                        \
        if (dg.vec4) hipLaunchKernelGGL((k_conv_bn_dir<KS, S, true>), grid, dim3(kDirTh), 0, st, x, w, bias, g, dg, a); \
        else hipLaunchKernelGGL((k_conv_bn_dir<KS, S, false>), grid, dim3(kDirTh), 0, st, x, w, bias, g, dg, a);     \
    } while (0)
    if (g.k == 3 && g.stride == 1) LRS_DIR(3, 1);
    else if (g.k == 3) LRS_DIR(3, 2);
    else if (g.stride == 1) LRS_DIR(1, 1);
    else LRS_DIR(1, 2);
#undef LRS_DIR
}

int sn_launch(const SnConv *table_dev, int n, int64_t max_elems, double *gram, float *sigma, float *scale,
              float ln_lambda, bool apply, hipStream_t st, long long *prof = nullptr) {
    hipLaunchKernelGGL(k_sn_gram, dim3(kSnSplit, n), dim3(256), 0, st, table_dev, gram);
    hipLaunchKernelGGL(k_sn_gram_reduce, dim3(kSnPairs, n), dim3(256), 0, st, table_dev, gram);
    hipLaunchKernelGGL(k_sn_sigma, dim3(n), dim3(256), 0, st, table_dev, gram, sigma, scale, ln_lambda, prof);
    if (apply) hipLaunchKernelGGL(k_sn_apply, dim3(ew_blocks(max_elems, 256), n), dim3(kEw), 0, st, table_dev, scale);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

// cr: the update reads the interior of a framed output (N = C cr->H cr->W elements of it)
int es_update(const float *out, int64_t N, float *ring, lrs_es_state *es, hipStream_t st, const EsCrop *cr = nullptr) {
    const unsigned nblk = ew_blocks(N, kEsMaxBlocks);
    if (cr) {
        if (N > INT32_MAX) return LRS_E_UNSUPPORTED;   // k_es_step_crop's 32-bit index map
        hipLaunchKernelGGL(k_es_step_crop, dim3(nblk), dim3(kEw), 0, st, out, N, ring, es, *cr);
    } else {
        hipLaunchKernelGGL(k_es_step, dim3(nblk), dim3(kEw), 0, st, out, N, ring, es);
    }
    hipLaunchKernelGGL(k_es_decide, dim3(1), dim3(64), 0, st, (const float *)ring, N, (int)nblk, es);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

}  // namespace

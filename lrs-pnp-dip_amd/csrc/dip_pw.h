// Pointwise (1x1, stride 1, unpadded) conv product of the DIP engine on the split-bf16 matrix cores, with
// the fused masked-MSE loss head of a network's last conv and the two kernels that reduce its sums.
#pragma once

#include "dip_kernels.h"   // act_fwd / act_bwd, block_sum2_d
#include "dip_gemm.h"      // s3_rsrc / s3_bload, kOob

namespace lrs {

// C[M][N] (+)= A[M][Kp] B[K][N] (+ bias[M]) for M <= 256 output channels over N pixels: the
// forward (A = the k_conv_prep forward planes WF, B = x) and the data gradient (A = WD = W^T planes,
// B = dL/dz) of the reference's 1x1 convs (my_Lipschitz_Unet.py:96-103, skip.py's 1x1 skips).
// One workgroup per 64 pixels: their B columns (all K) are read from HBM once and split into the
// three bf16 planes in LDS ([plane][pixel][k], row stride ldsrow bytes = 16 mod 256 so the 16
// pixel rows of a fragment read sit in distinct bank groups); the pre-split A fragments stream
// from L2 (one k-step prefetched), so every C element of the 64 pixels is produced by this one
// workgroup: no split-K, no tile quantisation on M.  Wave w owns rows 16 w + 64 j (j < MT).
struct PwArgs {
    const __bf16 *A;
    int64_t pstride;   // plane stride of A (elements)
    int lda;           // A row length (Kp, multiple of 16; columns >= the valid K are zero)
    const float *B;
    int K;             // valid B rows
    int64_t N;
    float *C;
    const float *bias;
    int M, Kp32, ldsrow, accum;
    int act;   // activation applied after the bias (a conv without BN: its act in the epilogue)
    // the masked-MSE head fused into the network's last conv (tgt != NULL; k_mse_head's arithmetic per
    // element): gz = act'(out) * (-norm (tgt m - out m) m) stored beside out, and per output row the
    // workgroup's fp64 sums of gz and of (tgt m - out m)^2 in hpart[0 / 1][row][blockIdx.x].  The mask
    // of output row m is read at m * mstride + n: mstride 0 for a [N] pixel mask, N for a per-element
    // [M][N] one (read like tgt)
    const float *tgt = nullptr, *msk = nullptr;
    int64_t mstride = 0;
    float *gz = nullptr;
    double *hpart = nullptr;
    float hnorm = 0.0f;
};

inline int pw_ldsrow(int Kp32) {   // bytes; Kp32 * 2 rounded up to 16 mod 256
    int b = Kp32 * 2;
    return b + (((16 - b) % 256) + 256) % 256;
}

// NB = 16-pixel column blocks per workgroup (16 NB pixels): 4, or 5, chosen per launch by
// pw_launch (dip_launch.h) from the rounds of CU slots the grid needs.
template <int MT, int NB = 4>
__global__ __launch_bounds__(256, 2) void k_pw(PwArgs a) {
    extern __shared__ __attribute__((aligned(16))) char pw_smem[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, jl = lane & 15, gk = lane >> 4;
    constexpr int NPX = 16 * NB;
    const int64_t n0 = (int64_t)blockIdx.x * NPX;
    const int64_t plane = (int64_t)NPX * a.ldsrow;
    if constexpr (NB == 4) {   // stage: thread (n = t & 63) splits k chunks (t >> 6) + 4 i of 8 values each.  Buffer
        // loads, branch-free: k (wave-uniform) goes in the scalar offset, so rows k >= K fall past
        // the buffer's K * N floats and read 0; a pixel n >= N reads at kOob.
        const int n = t & 63;
        const __amdgpu_buffer_rsrc_t rs = s3_rsrc(a.B, (int)(a.K * a.N * 4));
        const int voff = n0 + n < a.N ? (int)((n0 + n) * 4) : kOob;
        const int nck = a.Kp32 / 8, c0 = __builtin_amdgcn_readfirstlane(t >> 6);
        float v[8][8];   // all of the thread's chunks (<= 8 for K <= 256) in flight together
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = c0 + 4 * i;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t so = (int64_t)(8 * c + u) * a.N * 4;
                v[i][u] = c < nck ? s3_bload(rs, voff, so < kOob ? (int)so : kOob) : 0.0f;
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = c0 + 4 * i;
            if (c >= nck) break;
            bf16x8 p0, p1, p2;
            split_bf16x8(v[i], p0, p1, p2);
            char *dst = pw_smem + (int64_t)n * a.ldsrow + 16 * c;
            *reinterpret_cast<bf16x8 *>(dst) = p0;
            *reinterpret_cast<bf16x8 *>(dst + plane) = p1;
            *reinterpret_cast<bf16x8 *>(dst + 2 * plane) = p2;
        }
    } else {   // NPX pixels x nck chunks as items it = t + 256 j: pixel it % NPX, chunk it / NPX
        const __amdgpu_buffer_rsrc_t rs = s3_rsrc(a.B, (int)(a.K * a.N * 4));
        const int nck = a.Kp32 / 8, items = NPX * nck;
        constexpr int kMaxIt = (NPX * 32 + 255) / 256;   // K <= 256
        float v[kMaxIt][8];
#pragma unroll
        for (int j = 0; j < kMaxIt; ++j) {
            const int it = t + 256 * j, n = it % NPX, c = it / NPX;
            const int voff = n0 + n < a.N ? (int)((n0 + n) * 4) : kOob;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t so = (int64_t)(8 * c + u) * a.N * 4;
                v[j][u] = it < items ? s3_bload(rs, voff, so < kOob ? (int)so : kOob) : 0.0f;
            }
        }
#pragma unroll
        for (int j = 0; j < kMaxIt; ++j) {
            const int it = t + 256 * j, n = it % NPX, c = it / NPX;
            if (it >= items) break;
            bf16x8 p0, p1, p2;
            split_bf16x8(v[j], p0, p1, p2);
            char *dst = pw_smem + (int64_t)n * a.ldsrow + 16 * c;
            *reinterpret_cast<bf16x8 *>(dst) = p0;
            *reinterpret_cast<bf16x8 *>(dst + plane) = p1;
            *reinterpret_cast<bf16x8 *>(dst + 2 * plane) = p2;
        }
    }
    floatx4 acc[MT][NB];
#pragma unroll
    for (int j = 0; j < MT; ++j)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[j][b] = floatx4{0.f, 0.f, 0.f, 0.f};
    const int ksteps = a.Kp32 / 32;
    bf16x8 fa[MT][3], fn[MT][3];
    // A fragments: 16-B buffer loads (L2-resident planes), rows >= M and k >= lda at kOob (zeros)
    const __amdgpu_buffer_rsrc_t ra = s3_rsrc(a.A, (int)(3 * a.pstride * 2));
    auto loadA = [&](int ks, bf16x8 (&f)[MT][3]) {
        const int k = ks * 32 + 8 * gk;
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            const int row = 16 * wv + 64 * j + jl;
            const int vo = (row < a.M && k < a.lda) ? 2 * (row * a.lda + k) : kOob;
#pragma unroll
            for (int p = 0; p < 3; ++p)
                f[j][p] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(ra, vo, (int)(2 * p * a.pstride), 0));
        }
    };
    // NB = 4 prefetches the next k-step's A fragments; NB = 5 has no registers for that (its loads
    // overlap the step's B fragment reads from LDS instead)
    constexpr bool PF = NB == 4;
    loadA(0, fa);
    __syncthreads();
    for (int ks = 0; ks < ksteps; ++ks) {
        if constexpr (PF) {
            if (ks + 1 < ksteps) loadA(ks + 1, fn);
        } else if (ks > 0) {
            loadA(ks, fa);
        }
        bf16x8 fb[NB][3];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const char *s0 = pw_smem + (int64_t)(16 * b + jl) * a.ldsrow + 16 * (4 * ks + gk);
#pragma unroll
            for (int p = 0; p < 3; ++p) fb[b][p] = *reinterpret_cast<const bf16x8 *>(s0 + p * plane);
        }
#pragma unroll
        for (int j = 0; j < MT; ++j)
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[j][b] = split_mfma6(fa[j], fb[b], acc[j][b]);
        if (PF && ks + 1 < ksteps) {
#pragma unroll
            for (int j = 0; j < MT; ++j)
#pragma unroll
                for (int p = 0; p < 3; ++p) fa[j][p] = fn[j][p];
        }
    }
    // epilogue through LDS (the B image is dead after this barrier): wave w writes its 16 x 64 tile
    // of each row block as [row][pixel] and reads it back as float4 rows, so every 16 lanes store
    // one full 256-B pixel run of a channel row (the MFMA layout gives a lane 4 rows of 1 pixel)
    __syncthreads();
    constexpr int ES = NPX + 4;   // staging row stride (floats)
    float *E = reinterpret_cast<float *>(pw_smem) + wv * 16 * ES;
    const bool vec = (a.N & 3) == 0 && ((reinterpret_cast<uintptr_t>(a.C) & 15) == 0);
    const bool head = a.tgt != nullptr;
#pragma unroll
    for (int j = 0; j < MT; ++j) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) E[(4 * gk + r) * ES + 16 * b + jl] = acc[j][b][r];
        __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): this wave's LDS writes done (wave-local tile)
        __builtin_amdgcn_wave_barrier();
        double hs[NB], hb[NB];   // head: this lane's loss / bias-gradient sums of its run per i
#pragma unroll
        for (int i = 0; i < NB; ++i) {   // 16 rows x NPX / 4 float4 runs
            hs[i] = 0.0;
            hb[i] = 0.0;
            const int idx = lane + 64 * i, rr = idx / (4 * NB), q = 4 * (idx % (4 * NB));
            const int m = 16 * wv + 64 * j + rr;
            const int64_t n = n0 + q;
            if (m >= a.M) continue;
            float4 v = *reinterpret_cast<const float4 *>(E + rr * ES + q);
            const float bs = a.bias ? a.bias[m] : 0.0f;
            float *c = a.C + (int64_t)m * a.N + n;
            if (vec && n + 3 < a.N) {
                if (a.bias) { v.x = v.x + bs; v.y = v.y + bs; v.z = v.z + bs; v.w = v.w + bs; }
                if (a.accum) {
                    const float4 o = *reinterpret_cast<const float4 *>(c);
                    v.x = o.x + v.x; v.y = o.y + v.y; v.z = o.z + v.z; v.w = o.w + v.w;
                }
                if (a.act) { v.x = act_fwd(v.x, a.act); v.y = act_fwd(v.y, a.act); v.z = act_fwd(v.z, a.act); v.w = act_fwd(v.w, a.act); }
                *reinterpret_cast<float4 *>(c) = v;
                if (head) {   // k_mse_head's per-element arithmetic, in the same order
                    const float4 tv = *reinterpret_cast<const float4 *>(a.tgt + (int64_t)m * a.N + n);
                    const float4 mv = a.msk ? *reinterpret_cast<const float4 *>(a.msk + (int64_t)m * a.mstride + n)
                                            : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
                    const float oe[4] = {v.x, v.y, v.z, v.w}, te[4] = {tv.x, tv.y, tv.z, tv.w}, me[4] = {mv.x, mv.y, mv.z, mv.w};
                    float ge[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float d = te[e] * me[e] - oe[e] * me[e];
                        hs[i] += (double)d * (double)d;
                        ge[e] = act_bwd((-(a.hnorm * d)) * me[e], oe[e], a.act);
                        hb[i] += (double)ge[e];
                    }
                    *reinterpret_cast<float4 *>(a.gz + (int64_t)m * a.N + n) = make_float4(ge[0], ge[1], ge[2], ge[3]);
                }
            } else {
                const float vv[4] = {v.x, v.y, v.z, v.w};
                for (int u = 0; u < 4; ++u) {
                    if (n + u >= a.N) break;
                    float x = vv[u];
                    if (a.bias) x = x + bs;
                    if (a.accum) x = c[u] + x;
                    if (a.act) x = act_fwd(x, a.act);
                    c[u] = x;
                    if (head) {
                        const float mk = a.msk ? a.msk[(int64_t)m * a.mstride + n + u] : 1.0f;
                        const float d = a.tgt[(int64_t)m * a.N + n + u] * mk - x * mk;
                        hs[i] += (double)d * (double)d;
                        const float g = act_bwd((-(a.hnorm * d)) * mk, x, a.act);
                        a.gz[(int64_t)m * a.N + n + u] = g;
                        hb[i] += (double)g;
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (head) {   // each row's sums over the workgroup's runs, in run order, through this wave's LDS
            double2 *R = reinterpret_cast<double2 *>(E);   // [16 rows x 4 NB runs] (fits the wave's E)
            static_assert(16 * 4 * NB * sizeof(double2) <= 16 * ES * sizeof(float), "head sums fit the staging");
#pragma unroll
            for (int i = 0; i < NB; ++i) R[lane + 64 * i] = make_double2(hs[i], hb[i]);
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_wave_barrier();
            const int m = 16 * wv + 64 * j + lane;
            if (lane < 16 && m < a.M) {
                double sl = 0.0, sg = 0.0;
                for (int k = 0; k < 4 * NB; ++k) {
                    const double2 p = R[lane * 4 * NB + k];
                    sl += p.x;
                    sg += p.y;
                }
                a.hpart[(int64_t)m * gridDim.x + blockIdx.x] = sg;
                a.hpart[((int64_t)a.M + m) * gridDim.x + blockIdx.x] = sl;
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// The fused head's sums (k_pw with PwArgs::tgt): per channel c (grid C) the gz sums of the nwg
// workgroups, summed in a fixed order -> the conv's bias gradient, and the loss sums -> closs[c];
// k_head_loss then adds closs in channel order into loss_acc (deterministic, as k_mse_head).
__global__ __launch_bounds__(256) void k_head_reduce(const double *__restrict__ hpart, int C, int nwg, float *gbias,
                                                     double *closs) {
    __shared__ double red[12];
    const int c = blockIdx.x;
    double sg = 0.0, sl = 0.0;
    for (int w = threadIdx.x; w < nwg; w += blockDim.x) {
        sg += hpart[(int64_t)c * nwg + w];
        sl += hpart[((int64_t)C + c) * nwg + w];
    }
    block_sum2_d(sg, sl, red);
    if (threadIdx.x == 0) {
        gbias[c] = (float)sg;
        closs[c] = sl;
    }
}

__global__ void k_head_loss(const double *__restrict__ closs, int C, double *loss_acc) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += closs[c];
    *loss_acc += s;
}

}  // namespace lrs

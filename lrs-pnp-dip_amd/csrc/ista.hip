// Fused masked ISTA over every block of the unfolded cube: the dictionary-resident kernels and the
// dispatch of lrs_ista_f32.
//
// Reference path (shuoli0708/LRS-PnP-DIP): the per-block Python loop of main_LRS_PnP.py:270-303
// (…1-LiP.py:367-392) calling ista() (main_LRS_PnP.py:131-149 / …1-LiP.py:185-198) on the pruned
// dictionary (delete_element, :152-155), then Phi_z[:,jj] = Full_Dictionary @ Coefs.
//
// Which kernel serves a call of lrs_ista_f32 (first match):
//
//   n_pad, K                      prox              precision            kernel
//   K > 512, or ALGO_GENERIC      every             fp32-accurate GEMMs  ista_generic (ista_generic.hip)
//   n_pad <= 64 and K = 256       NLM (skimage)     split-bf16 (default) k_ista_ln2<256, 1>
//   n_pad <= 64 and K = 256       soft              split-bf16 (default) k_ista_b3<256>
//   n_pad <= 64 and K = 256       NLM (skimage)     f32                  k_ista_res<256, false>
//   n_pad <= 64 and K = 256       soft              f32                  k_ista_res<256, true>
//   any other n, K <= 512         every             f32                  k_ista_rs (ista_rs.hip)
//   (NLM (MATLAB) at every shape runs k_ista_rs; blocks that share observation patterns have their
//    own entry, lrs_ista_pat_f32 -> k_ista_pat, ista_pat.hip)
//
// Common to the three resident kernels of this file (n_pad <= 64, i.e. bb <= 8):
//  * blocks are the GEMM N dimension: one wave owns 16 blocks (one MFMA column tile);
//  * pruning becomes masking: H^T(y - Hx) == D^T(m .* (y - Dx)) with m the observed-row mask;
//  * the dictionary is staged in LDS once per workgroup and stays for the kernel's lifetime; y, the
//    row mask and the coefficients stay in VGPRs for all Nit iterations.  Both products per inner
//    iteration run on MFMA: R = m.*(y - D x) (M = rows, K = atoms), then G = D^T R (M = atoms,
//    K = rows); the accumulator of each product is directly the B operand of the next one, so
//    nothing crosses LDS but D;
//  * the NLM prox runs in fp64 on the accumulator layout (a lane holds 4 consecutive atoms per tile).
#include "ista_paths.h"
#include "lrs_nlm.h"
#include "lrs_split.h"

namespace lrs {

constexpr int kIstaWaves = 8;
constexpr int kIstaThreads = kIstaWaves * kWave;
constexpr int kStageRows = 64;

template <int K>
struct alignas(16) IstaSmem {
    float DA[kStageRows][K + 4];  // [row][atom]; +4 keeps b128 rows aligned, spreads banks
    float DT[K][kStageRows + 4];  // [atom][row]
};

// a / b from the correctly rounded reciprocal y = 1/b with one Markstein correction step:
// q = a*y, r = fma(-b, q, a) (exact), q + r*y.  Equals the IEEE quotient a/b (the reference's
// torch division) away from overflow/underflow, at 3 instructions instead of ~10.
__device__ __forceinline__ float div_by(float a, float b, float y) {
    const float q = a * y;
    const float r = __fmaf_rn(-b, q, a);
    return __fmaf_rn(r, y, q);
}

struct IstaParams {
    const float *Yb;
    const uint8_t *obs;
    const float *D;
    const float *alpha;
    const double *thr;
    float *coefs;
    float *phi;
    int n, n_pad, Nit, prox;
    int64_t nb;
    double seven;   // 7.0, passed in so fma(7, x, c) keeps its addend in place (no per-use copy)
};

template <int K>
__device__ __forceinline__ void stage_dictionary(IstaSmem<K> &S, const float *__restrict__ D, int n) {
    for (int idx = threadIdx.x; idx < kStageRows * K; idx += kIstaThreads) {
        const int r = idx / K, a = idx % K;
        const float v = r < n ? D[(int64_t)r * K + a] : 0.0f;
        S.DA[r][a] = v;
        S.DT[a][r] = v;
    }
}

// The 4 NLM outputs of one chunk; w[0..10] = v-hat[a0-3 .. a0+7] (a0 = first atom of chunk).
// Each symmetric weight w(i,+t) == w(i+t,-t) is computed once: 18 weights for 4 outputs.
__device__ __forceinline__ void nlm_chunk(const double (&w)[11], double kneg, double c0, float (&out)[4]) {
    int W1[7], W2[7], W3[7];      // W_t[i] = hi word of w(a0-3+i, +t), s_t[i] = (w[i] - w[i+t])^2
    {
        double sp = (w[2] - w[3]) * (w[2] - w[3]);
#pragma unroll
        for (int i = 2; i < 7; ++i) {
            const double d = w[i + 1] - w[i + 2], sn = d * d;
            W1[i] = nlm_weight_hi(sp + sn, kneg);
            sp = sn;
        }
    }
    {
        double sp = (w[1] - w[3]) * (w[1] - w[3]);
#pragma unroll
        for (int i = 1; i < 7; ++i) {
            const double d = w[i + 1] - w[i + 3], sn = d * d;
            W2[i] = nlm_weight_hi(sp + sn, kneg);
            sp = sn;
        }
    }
    {
        double sp = (w[0] - w[3]) * (w[0] - w[3]);
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            const double d = w[i + 1] - w[i + 4], sn = d * d;
            W3[i] = nlm_weight_hi(sp + sn, kneg);
            sp = sn;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int C = 3 + e;
        // t = -3,-2,-1,+1,+2,+3 (the canonical order of oracle_nlm_col)
        const double ws[6] = {hi_to_double(W3[C - 3]), hi_to_double(W2[C - 2]), hi_to_double(W1[C - 1]),
                              hi_to_double(W1[C]), hi_to_double(W2[C]), hi_to_double(W3[C])};
        const double vs[6] = {w[C - 3], w[C - 2], w[C - 1], w[C + 1], w[C + 2], w[C + 3]};
        double sw = 0.0, swv = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            sw = sw + ws[k];
            swv = __fma_rn(ws[k], vs[k], swv);
        }
        const double num = __fma_rn(7.0, swv, c0 * w[C]);
        const double den = __fma_rn(7.0, sw, c0);
        out[e] = (float)(num / den);
    }
}

// Neighbour-exchange state for the in-register NLM along the atom axis.  A lane (block l&15,
// group g = l>>4) holds atoms 16q+4g .. 16q+4g+3 of every 16-atom tile q; chunk c-1 lives in
// lane l-16 (same tile, or tile q-1 when g == 0), chunk c+1 in lane l+16 (tile q+1 when g == 3).
struct NlmLanes {
    int g, src_prev, src_next;
    __device__ __forceinline__ explicit NlmLanes(int lane)
        : g(lane >> 4), src_prev((lane + 48) & 63), src_next((lane + 16) & 63) {}
};

// NLM of tile q given this lane's gradient chunk `own`, the shuffled neighbours of tiles q-1/q/q+1
// (Pprev = prev-lane chunk of tile q-1, Pcur = of tile q; Ncur = next-lane chunk of tile q,
// Nnext = of tile q+1), with numpy-style reflection at both ends of the K atoms.
template <int NQ>
__device__ __forceinline__ void nlm_tile(int q, const NlmLanes &L, const float (&own)[4], const float (&Pprev)[3],
                                         const float (&Pcur)[3], const float (&Ncur)[4], const float (&Nnext)[4],
                                         double kneg, double c0, float (&out)[4]) {
    float prv[3], nxt[4];
    if (L.g == 0) {
        if (q == 0) { prv[0] = own[3]; prv[1] = own[2]; prv[2] = own[1]; }   // reflect
        else { prv[0] = Pprev[0]; prv[1] = Pprev[1]; prv[2] = Pprev[2]; }
    } else {
        prv[0] = Pcur[0]; prv[1] = Pcur[1]; prv[2] = Pcur[2];
    }
    if (L.g == 3) {
        if (q == NQ - 1) { nxt[0] = own[2]; nxt[1] = own[1]; nxt[2] = own[0]; nxt[3] = prv[2]; }
        else { nxt[0] = Nnext[0]; nxt[1] = Nnext[1]; nxt[2] = Nnext[2]; nxt[3] = Nnext[3]; }
    } else {
        nxt[0] = Ncur[0]; nxt[1] = Ncur[1]; nxt[2] = Ncur[2]; nxt[3] = Ncur[3];
    }
    const double w[11] = {prv[0], prv[1], prv[2], own[0], own[1], own[2], own[3],
                          nxt[0], nxt[1], nxt[2], nxt[3]};
    nlm_chunk(w, kneg, c0, out);
}

// ------------------------------------------------------------------------------------------------
// f32 resident kernel: exact f32 products on v_mfma_f32_16x16x4_f32.  A 512-thread workgroup owns 128
// blocks, 2 waves per SIMD so one wave's fp64 NLM overlaps the other's MFMA.  D is staged in two
// images, [row][atom] for the first product and [atom][row] for the second, both read with
// ds_read_b128 (4 k-steps per read); the NLM neighbours a lane needs (3 + 4 atoms) come from lanes
// l-16 / l+16.  A software pipeline runs over the 16 atom tiles q of each inner iteration:
//     MFMA : G[q+2] = D^T r (tile q+2)        | VALU : NLM of tile q -> x_new[q]
//     MFMA : R_next += D[:, tile q] x_new[q]  | VALU : g[q+2] = x[q+2] + G[q+2]/alpha
// so the matrix pipe works on the next products while the fp64 NLM of the current tile runs.
// R_next = D x_new is complete when the last tile is done: it is the next iteration's residual
// input and, after the last iteration, Phi = D x.
// ------------------------------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ floatx4 gemm2_tile(const IstaSmem<K> &S, int q, const float (&r)[4][4], int jl, int g) {
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float4 a = *reinterpret_cast<const float4 *>(&S.DT[16 * q + jl][16 * t + 4 * g]);
        acc = mfma16x16x4(a.x, r[t][0], acc);
        acc = mfma16x16x4(a.y, r[t][1], acc);
        acc = mfma16x16x4(a.z, r[t][2], acc);
        acc = mfma16x16x4(a.w, r[t][3], acc);
    }
    return acc;
}

template <int K>
__device__ __forceinline__ void gemm1_tile(const IstaSmem<K> &S, int q, const float (&x)[4], floatx4 (&R)[4], int jl,
                                           int g) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float4 a = *reinterpret_cast<const float4 *>(&S.DA[16 * t + jl][16 * q + 4 * g]);
        R[t] = mfma16x16x4(a.x, x[0], R[t]);
        R[t] = mfma16x16x4(a.y, x[1], R[t]);
        R[t] = mfma16x16x4(a.z, x[2], R[t]);
        R[t] = mfma16x16x4(a.w, x[3], R[t]);
    }
}

template <int K, bool SOFT>
__global__ __launch_bounds__(kIstaThreads, 2) void k_ista_res(IstaParams p) {
    constexpr int NQ = K / 16;
    __shared__ __attribute__((aligned(16))) IstaSmem<K> S;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int jl = lane & 15, g = lane >> 4;
    const int64_t j = ((int64_t)blockIdx.x * kIstaWaves + wave) * 16 + jl;
    const bool valid = j < p.nb;
    const int NT = p.n_pad / 16;
    const NlmLanes L(lane);

    const float alpha = valid ? p.alpha[j] : 1.0f;
    const double thr = valid ? p.thr[j] : 1.0;
    const double kneg = nlm_kneg(thr);
    const double c0 = nlm_c0();
    const float Tsoft = (float)thr;

    float y[4][4];
    uint32_t mres = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float4 yv = {0.f, 0.f, 0.f, 0.f};
        uint32_t mv = 0;
        if (valid && t < NT) {
            yv = *reinterpret_cast<const float4 *>(&p.Yb[j * p.n_pad + 16 * t + 4 * g]);
            mv = *reinterpret_cast<const uint32_t *>(&p.obs[j * p.n_pad + 16 * t + 4 * g]);
        }
        y[t][0] = yv.x; y[t][1] = yv.y; y[t][2] = yv.z; y[t][3] = yv.w;
#pragma unroll
        for (int i = 0; i < 4; ++i) mres |= (((mv >> (8 * i)) & 0xffu) ? 1u : 0u) << (4 * t + i);
    }
    stage_dictionary<K>(S, p.D, p.n);
    __syncthreads();

    float X[NQ][4];
#pragma unroll
    for (int q = 0; q < NQ; ++q) X[q][0] = X[q][1] = X[q][2] = X[q][3] = 0.f;
    floatx4 R[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) R[t] = floatx4{0.f, 0.f, 0.f, 0.f};   // D x for x = 0

    const float ainv = 1.0f / alpha;
    auto gradient = [&](floatx4 &Gq, const float (&xq)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) Gq[i] = xq[i] + div_by(Gq[i], alpha, ainv);   // x + (D^T r)/alpha
    };

    for (int it = 0; it < p.Nit; ++it) {
        float r[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int i = 0; i < 4; ++i) r[t][i] = ((mres >> (4 * t + i)) & 1u) ? (y[t][i] - R[t][i]) : 0.0f;
            R[t] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
        floatx4 G[NQ];
        // a closure on purpose: calling gemm2_tile directly changes the generated code
        auto gemm2 = [&](int q) -> floatx4 { return gemm2_tile<K>(S, q, r, jl, g); };
        G[0] = gemm2(0);
        G[1] = gemm2(1);
        __builtin_amdgcn_sched_barrier(0);
        gradient(G[0], X[0]);
        gradient(G[1], X[1]);
        float Pprev[3] = {0.f, 0.f, 0.f}, Pcur[3], Ncur[4], Nnext[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) Ncur[e] = __shfl(G[0][e], L.src_next, 64);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            if (q + 2 < NQ) G[q + 2] = gemm2(q + 2);
            const float own[4] = {G[q][0], G[q][1], G[q][2], G[q][3]};
            float o[4];
            if (SOFT) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float t = fabsf(own[i]) - Tsoft;
                    t = t > 0.f ? t : 0.f;
                    o[i] = own[i] > 0.f ? t : (own[i] < 0.f ? -t : 0.f);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 3; ++e) Pcur[e] = __shfl(G[q][e + 1], L.src_prev, 64);
                if (q + 1 < NQ) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) Nnext[e] = __shfl(G[q + 1][e], L.src_next, 64);
                }
                nlm_tile<NQ>(q, L, own, Pprev, Pcur, Ncur, Nnext, kneg, c0, o);
#pragma unroll
                for (int e = 0; e < 3; ++e) Pprev[e] = Pcur[e];
#pragma unroll
                for (int e = 0; e < 4; ++e) Ncur[e] = Nnext[e];
            }
            X[q][0] = o[0]; X[q][1] = o[1]; X[q][2] = o[2]; X[q][3] = o[3];
            gemm1_tile<K>(S, q, X[q], R, jl, g);
            if (q + 2 < NQ) gradient(G[q + 2], X[q + 2]);
            // keep each pipeline step's LDS reads and MFMAs inside the step: without this fence
            // the scheduler hoists every tile's ds_reads to the loop top and spills
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    if (valid) {
        if (p.coefs) {
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                *reinterpret_cast<float4 *>(&p.coefs[j * K + 16 * q + 4 * g]) =
                    make_float4(X[q][0], X[q][1], X[q][2], X[q][3]);
        }
        // Phi_z = Full_Dictionary @ Coefs == R (all rows, missing ones included)
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < NT)
                *reinterpret_cast<float4 *>(&p.phi[j * p.n_pad + 16 * t + 4 * g]) =
                    make_float4(R[t][0], R[t][1], R[t][2], R[t][3]);
    }
}

// ------------------------------------------------------------------------------------------------
// Split-bf16 resident kernel (n_pad <= 64, K = 256).  The two products per inner iteration are
// fp32-accurate products on the bf16 matrix cores (lrs_split.h: the split, the chain, the accuracy).
//   * D lives in LDS once, as three bf16 images [row][atom] with 8-byte chunks XOR-swizzled per
//     row; the first product reads its A fragments by rows (ds_read_b64), the second reads the
//     same images transposed (ds_read_b64_tr_b16): 96 KB instead of the f32 kernel's 136 KB;
//   * accumulators feed the next product's B operand directly (C rows 4g..4g+3 of two 16-tiles
//     = the 8 k-values of lane group g), as in the f32 kernel.
// ------------------------------------------------------------------------------------------------
typedef short short4v __attribute__((ext_vector_type(4)));

template <int K>
struct alignas(16) IstaSmemB3 {
    __bf16 D[3][kStageRows][K];   // split s of D, [row][atom], chunk-swizzled
};

// XOR swizzle of the 8-byte chunk index by row (linear over GF(2) in row & 15): conflict-free for
// the 32-lane halves of both the row reads and the transposed reads (searched exhaustively)
__device__ __forceinline__ int b3_swz(int row) {
    return ((row & 1) ? 26 : 0) ^ ((row & 2) ? 12 : 0) ^ ((row & 4) ? 62 : 0) ^ ((row & 8) ? 3 : 0);
}

template <int K>
__device__ __forceinline__ int b3_off(int row, int chunk) {   // element offset within one image
    return row * K + 4 * (chunk ^ b3_swz(row));
}

constexpr int kB3Waves = 4;                       // one wave per SIMD: the whole 512-entry register file
constexpr int kB3Threads = kB3Waves * kWave;

template <int K>
__device__ __forceinline__ void stage_dictionary_b3(IstaSmemB3<K> &S, const float *__restrict__ D, int n) {
    for (int idx = threadIdx.x; idx < kStageRows * K; idx += kB3Threads) {
        const int r = idx / K, a = idx % K;
        const float v = r < n ? D[(int64_t)r * K + a] : 0.0f;
        const Bf16Split s = split_bf16(v);
        const int o = b3_off<K>(r, a >> 2) + (a & 3);
        S.D[0][0][o] = s.b0;
        S.D[1][0][o] = s.b1;
        S.D[2][0][o] = s.b2;
    }
}

// 8 bf16 per split from 2 x 4 fp32 (elements 0..3 = u, 4..7 = w)
__device__ __forceinline__ void split_frag(const float (&u)[4], const float (&w)[4], bf16x8 (&f)[3]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const Bf16Split a = split_bf16(u[e]);
        f[0][e] = a.b0; f[1][e] = a.b1; f[2][e] = a.b2;
        const Bf16Split b = split_bf16(w[e]);
        f[0][e + 4] = b.b0; f[1][e + 4] = b.b1; f[2][e + 4] = b.b2;
    }
}

__device__ __forceinline__ bf16x8 cat4(bf16x4 a, bf16x4 b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7); }

// G tile q = D^T r: A = D^T rows (atoms 16q..16q+15) by transposed reads, B = r split, per row pair
template <int K>
__device__ __forceinline__ floatx4 b3_gemm2(const IstaSmemB3<K> &S, int q, const bf16x8 (&rf)[2][3], int lane) {
    const int g = lane >> 4, ll = lane & 15, qq = ll >> 2, pp = ll & 3;
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
        const int r0 = 32 * pr + 4 * g + qq, r1 = r0 + 16;
        bf16x8 A[3];
#pragma unroll
        for (int sp = 0; sp < 3; ++sp) {
            typedef __attribute__((address_space(3))) short4v lds_s4;
            const short4v a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (lds_s4 *)(&S.D[sp][0][b3_off<K>(r0, 4 * q + pp)]));
            const short4v a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (lds_s4 *)(&S.D[sp][0][b3_off<K>(r1, 4 * q + pp)]));
            A[sp] = cat4(__builtin_bit_cast(bf16x4, a0), __builtin_bit_cast(bf16x4, a1));
        }
        acc = split_mfma6(A, rf[pr], acc);
    }
    return acc;
}

// R[t] += D rows (16t..) x (atom tiles 2p, 2p+1): A = D rows by row reads, B = x split
template <int K>
__device__ __forceinline__ void b3_gemm1(const IstaSmemB3<K> &S, int p, const bf16x8 (&xf)[3], floatx4 (&R)[4],
                                         int lane) {
    const int g = lane >> 4, ll = lane & 15;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int row = 16 * t + ll;
        bf16x8 A[3];
#pragma unroll
        for (int sp = 0; sp < 3; ++sp) {
            const bf16x4 a0 = *reinterpret_cast<const bf16x4 *>(&S.D[sp][0][b3_off<K>(row, 8 * p + g)]);
            const bf16x4 a1 = *reinterpret_cast<const bf16x4 *>(&S.D[sp][0][b3_off<K>(row, 8 * p + 4 + g)]);
            A[sp] = cat4(a0, a1);
        }
        R[t] = split_mfma6(A, xf, R[t]);
    }
}

// The soft-threshold prox on the split-bf16 products (the NLM prox has its own kernel, k_ista_ln2).
template <int K>
__global__ __launch_bounds__(kB3Threads, 1) void k_ista_b3(IstaParams p) {
    static_assert(K == 256, "the chunk swizzle assumes 64 chunks per row");
    constexpr int NQ = K / 16;
    __shared__ __attribute__((aligned(16))) IstaSmemB3<K> S;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int jl = lane & 15, g = lane >> 4;
    const int64_t j = ((int64_t)blockIdx.x * kB3Waves + wave) * 16 + jl;
    const bool valid = j < p.nb;
    const int NT = p.n_pad / 16;

    const float alpha = valid ? p.alpha[j] : 1.0f;
    const float Tsoft = (float)(valid ? p.thr[j] : 1.0);

    float y[4][4];
    uint32_t mres = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float4 yv = {0.f, 0.f, 0.f, 0.f};
        uint32_t mv = 0;
        if (valid && t < NT) {
            yv = *reinterpret_cast<const float4 *>(&p.Yb[j * p.n_pad + 16 * t + 4 * g]);
            mv = *reinterpret_cast<const uint32_t *>(&p.obs[j * p.n_pad + 16 * t + 4 * g]);
        }
        y[t][0] = yv.x; y[t][1] = yv.y; y[t][2] = yv.z; y[t][3] = yv.w;
#pragma unroll
        for (int i = 0; i < 4; ++i) mres |= (((mv >> (8 * i)) & 0xffu) ? 1u : 0u) << (4 * t + i);
    }
    stage_dictionary_b3<K>(S, p.D, p.n);
    __syncthreads();

    float X[NQ][4];
#pragma unroll
    for (int q = 0; q < NQ; ++q) X[q][0] = X[q][1] = X[q][2] = X[q][3] = 0.f;
    floatx4 R[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) R[t] = floatx4{0.f, 0.f, 0.f, 0.f};

    const float ainv = 1.0f / alpha;
    auto gradient = [&](floatx4 &Gq, const float (&xq)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) Gq[i] = xq[i] + div_by(Gq[i], alpha, ainv);
    };

    for (int it = 0; it < p.Nit; ++it) {
        float r[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int i = 0; i < 4; ++i) r[t][i] = ((mres >> (4 * t + i)) & 1u) ? (y[t][i] - R[t][i]) : 0.0f;
            R[t] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
        bf16x8 rf[2][3];
        split_frag(r[0], r[1], rf[0]);
        split_frag(r[2], r[3], rf[1]);
        // pipeline over tile pairs: step p runs the products of tiles 2p+4, 2p+5 beside the prox of
        // tiles 2p and 2p+1 and their D x
        floatx4 G[NQ];
        // a closure on purpose: calling b3_gemm2 directly costs 14 more AGPRs
        auto gemm2 = [&](int q) -> floatx4 { return b3_gemm2<K>(S, q, rf, lane); };
#pragma unroll
        for (int q = 0; q < 4; ++q) G[q] = gemm2(q);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 4; ++q) gradient(G[q], X[q]);
#pragma unroll
        for (int pp = 0; pp < NQ / 2; ++pp) {
            const int qa = 2 * pp, qb = qa + 1;
            if (qa + 4 < NQ) G[qa + 4] = gemm2(qa + 4);
            if (qb + 4 < NQ) G[qb + 4] = gemm2(qb + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float t = fabsf(G[qa][i]) - Tsoft;
                t = t > 0.f ? t : 0.f;
                X[qa][i] = G[qa][i] > 0.f ? t : (G[qa][i] < 0.f ? -t : 0.f);
                float u = fabsf(G[qb][i]) - Tsoft;
                u = u > 0.f ? u : 0.f;
                X[qb][i] = G[qb][i] > 0.f ? u : (G[qb][i] < 0.f ? -u : 0.f);
            }
            bf16x8 xf[3];
            split_frag(X[qa], X[qb], xf);
            b3_gemm1<K>(S, pp, xf, R, lane);
            if (qa + 4 < NQ) gradient(G[qa + 4], X[qa + 4]);
            if (qb + 4 < NQ) gradient(G[qb + 4], X[qb + 4]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    if (valid) {
        if (p.coefs) {
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                *reinterpret_cast<float4 *>(&p.coefs[j * K + 16 * q + 4 * g]) =
                    make_float4(X[q][0], X[q][1], X[q][2], X[q][3]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < NT)
                *reinterpret_cast<float4 *>(&p.phi[j * p.n_pad + 16 * t + 4 * g]) =
                    make_float4(R[t][0], R[t][1], R[t][2], R[t][3]);
    }
}

// ---- split-bf16 kernel with the NLM prox: lane-contiguous atom layout, explicit schedule ---------
// The atom order inside the MFMA tiles is free (it is the A operand's row choice), so tile q row
// 4g+i holds atom 64g + 4q + i: lane group g owns the 64 consecutive atoms 64g .. 64g+63 across its
// 16 tiles.  The NLM neighbours of a chunk are then the lane's own previous / next tile, except at
// the group edges (tile 0's left and tile 15's right neighbours: 7 shuffles per iteration).
// Chunk c's weights W1[2], W2[1..2], W3[0..2] (pairs starting left of the chunk) equal chunk c-1's
// W1[6], W2[5..6], W3[4..6], so a lane computes 12 of the 18 weights and carries the other 6 over
// from its previous chunk; they are bitwise nlm_chunk's.  The weight sums are exact in fp64 (<= 6
// terms of 21 significant bits within 8 binades), so their order is free; num / den is a Newton
// step on v_rcp_f64 (|error| < 1 ulp of fp64 before the final float rounding).
// Per iteration: prologue (residual, tiles 0..3 and the edge copy of tile 15), then 8 steps of 4
// slots.  Slot k of step p runs one NLM phase (weights / outputs of chunk 2p, then of 2p+1) beside
// the MFMAs of up to two 6-MFMA units (a gemm2 tile half or a gemm1 row tile) whose LDS operands
// the previous slot loaded, and loads the next slot's operands.
struct Frag3 {
    bf16x8 a[3];
};

// Tile-major image: chunk c = 16 p' + q' of row r at element q' * 1024 + r * 16 + 4 (p' ^ s(r)),
// s(r) = 2 ((r >> 3) & 1).  Every read of a tile / row tile is a lane-constant base plus an
// immediate (no per-read address VALU), and both read kinds are conflict-free per 32-lane half.
__device__ __forceinline__ int tm_off(int row, int chunk) {
    return (chunk & 15) * 1024 + row * 16 + 4 * ((chunk >> 4) ^ (((row >> 3) & 1) << 1));
}

template <int K>
__device__ __forceinline__ void stage_dictionary_tm(IstaSmemB3<K> &S, const float *__restrict__ D, int n) {
    for (int idx = threadIdx.x; idx < kStageRows * K; idx += kB3Threads) {
        const int r = idx / K, a = idx % K;
        const float v = r < n ? D[(int64_t)r * K + a] : 0.0f;
        const Bf16Split s = split_bf16(v);
        const int o = tm_off(r, a >> 2) + (a & 3);
        S.D[0][0][o] = s.b0;
        S.D[1][0][o] = s.b1;
        S.D[2][0][o] = s.b2;
    }
}

struct TmLane {
    int tr, g1;   // lane-constant element offsets of the transposed and the row reads
    __device__ __forceinline__ explicit TmLane(int lane) {
        const int g = lane >> 4, ll = lane & 15, qq = ll >> 2, pp = ll & 3, rt = 4 * g + qq;
        tr = rt * 16 + 4 * (pp ^ (((rt >> 3) & 1) << 1));
        g1 = ll * 16 + 4 * (g ^ (((ll >> 3) & 1) << 1));
    }
};

template <int K>
__device__ __forceinline__ void tm_load_g2(const IstaSmemB3<K> &S, int q, int pr, const TmLane &A, Frag3 &F) {
#pragma unroll
    for (int sp = 0; sp < 3; ++sp) {
        typedef __attribute__((address_space(3))) short4v lds_s4;
        const __bf16 *b = &S.D[sp][0][0] + A.tr + q * 1024 + pr * 512;
        const short4v a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4 *)b);
        const short4v a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4 *)(b + 256));
        F.a[sp] = cat4(__builtin_bit_cast(bf16x4, a0), __builtin_bit_cast(bf16x4, a1));
    }
}

template <int K>
__device__ __forceinline__ void tm_load_g1(const IstaSmemB3<K> &S, int t, int p, const TmLane &A, Frag3 &F) {
#pragma unroll
    for (int sp = 0; sp < 3; ++sp) {
        const __bf16 *b = &S.D[sp][0][0] + A.g1 + 2 * p * 1024 + t * 256;
        const bf16x4 a0 = *reinterpret_cast<const bf16x4 *>(b);
        const bf16x4 a1 = *reinterpret_cast<const bf16x4 *>(b + 1024);
        F.a[sp] = cat4(a0, a1);
    }
}

// unit u (0/1) of slot k of step pp: kind 0 none, 1 gemm2 (tile a, half b), 2 gemm1 (row tile a, pair b)
struct LnUnit {
    int kind, a, b;
};
__device__ constexpr LnUnit ln_unit(int pp, int k, int u) {
    if (pp < 0 || pp > 7) return {0, 0, 0};
    if (pp == 0) return u == 0 ? LnUnit{1, 4 + (k >> 1), k & 1} : LnUnit{0, 0, 0};
    if (pp >= 6) return u == 0 ? LnUnit{2, k, pp - 1} : LnUnit{0, 0, 0};
    const int idx = 2 * k + u;      // 0..3 gemm2 halves of tiles 2pp+4, 2pp+5; 4..7 gemm1 row tiles
    if (idx < 4) return {1, 2 * pp + 4 + (idx >> 1), idx & 1};
    return {2, idx - 4, pp - 1};
}

template <int K>
__device__ __forceinline__ void ln_load_unit(const IstaSmemB3<K> &S, LnUnit U, const TmLane &A, Frag3 &F) {
    if (U.kind == 1) tm_load_g2<K>(S, U.a, U.b, A, F);
    else if (U.kind == 2) tm_load_g1<K>(S, U.a, U.b, A, F);
}

// whole-tile products through the unit loaders (prologue / epilogue)
template <int K>
__device__ __forceinline__ floatx4 tm_gemm2(const IstaSmemB3<K> &S, int q, const bf16x8 (&rf)[2][3], const TmLane &A) {
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
        Frag3 F;
        ln_load_unit<K>(S, LnUnit{1, q, pr}, A, F);
        acc = split_mfma6(F.a, rf[pr], acc);
    }
    return acc;
}

template <int K>
__device__ __forceinline__ void tm_gemm1(const IstaSmemB3<K> &S, int p, const bf16x8 (&xf)[3], floatx4 (&R)[4],
                                         const TmLane &A) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        Frag3 F;
        ln_load_unit<K>(S, LnUnit{2, t, p}, A, F);
        R[t] = split_mfma6(F.a, xf, R[t]);
    }
}

// DIV: the quotient of nlm_outputs (lrs_nlm.h): 1 = the Newton step, 0 = the bare reciprocal
template <int K, int DIV>
__global__ __launch_bounds__(kB3Threads, 1) void k_ista_ln2(IstaParams p) {
    static_assert(K == 256, "the lane layout assumes 4 groups of 64 atoms");
    // 1/alpha is folded into the residual before D^T.  The unfolded arm of `gradient` is never
    // taken; it stays because the closure then captures alpha and ainv, and without that capture
    // the compiler emits different code for this kernel (the same fragility as the twin
    // instantiation below).
    constexpr bool FOLD = true;
    constexpr int NQ = K / 16;
    __shared__ __attribute__((aligned(16))) IstaSmemB3<K> S;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int jl = lane & 15, g = lane >> 4;
    const int64_t j = ((int64_t)blockIdx.x * kB3Waves + wave) * 16 + jl;
    const bool valid = j < p.nb;
    const int NT = p.n_pad / 16;
    const int src_prev = (lane + 48) & 63, src_next = (lane + 16) & 63;
    const TmLane AL(lane);

    const float alpha = valid ? p.alpha[j] : 1.0f;
    const double thr = valid ? p.thr[j] : 1.0;
    const double kneg = nlm_kneg(thr);
    const double c0 = nlm_c0();

    float y[4][4];
    uint32_t mres = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float4 yv = {0.f, 0.f, 0.f, 0.f};
        uint32_t mv = 0;
        if (valid && t < NT) {
            yv = *reinterpret_cast<const float4 *>(&p.Yb[j * p.n_pad + 16 * t + 4 * g]);
            mv = *reinterpret_cast<const uint32_t *>(&p.obs[j * p.n_pad + 16 * t + 4 * g]);
        }
        y[t][0] = yv.x; y[t][1] = yv.y; y[t][2] = yv.z; y[t][3] = yv.w;
#pragma unroll
        for (int i = 0; i < 4; ++i) mres |= (((mv >> (8 * i)) & 0xffu) ? 1u : 0u) << (4 * t + i);
    }
    stage_dictionary_tm<K>(S, p.D, p.n);
    __syncthreads();

    float X[NQ][4];   // X[q][i] = coefficient of atom 64g + 4q + i
#pragma unroll
    for (int q = 0; q < NQ; ++q) X[q][0] = X[q][1] = X[q][2] = X[q][3] = 0.f;
    floatx4 R[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) R[t] = floatx4{0.f, 0.f, 0.f, 0.f};

    const float ainv = 1.0f / alpha;
    auto gradient = [&](floatx4 &Gq, const float (&xq)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) Gq[i] = FOLD ? xq[i] + Gq[i] : xq[i] + div_by(Gq[i], alpha, ainv);
    };

    for (int it = 0; it < p.Nit; ++it) {
        float r[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                r[t][i] = ((mres >> (4 * t + i)) & 1u) ? (y[t][i] - R[t][i]) : 0.0f;
                if (FOLD) r[t][i] = div_by(r[t][i], alpha, ainv);   // D^T (r / alpha)
            }
            R[t] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
        bf16x8 rf[2][3];
        split_frag(r[0], r[1], rf[0]);
        split_frag(r[2], r[3], rf[1]);
        floatx4 G[NQ];
        float edge_prev[3], edge_next[4];
        {
            floatx4 G15 = tm_gemm2<K>(S, NQ - 1, rf, AL);
#pragma unroll
            for (int q = 0; q < 4; ++q) G[q] = tm_gemm2<K>(S, q, rf, AL);
            gradient(G15, X[NQ - 1]);
#pragma unroll
            for (int q = 0; q < 4; ++q) gradient(G[q], X[q]);
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const float v = __shfl(G15[e + 1], src_prev, 64);
                edge_prev[e] = (g == 0) ? G[0][3 - e] : v;      // reflect: atoms -3,-2,-1 -> 3,2,1
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) edge_next[e] = __shfl(G[0][e], src_next, 64);
        }
        Frag3 F[2][2];
        ln_load_unit<K>(S, ln_unit(0, 0, 0), AL, F[0][0]);
        ln_load_unit<K>(S, ln_unit(0, 0, 1), AL, F[0][1]);
        __builtin_amdgcn_sched_barrier(0);

        int carry[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int pp = 0; pp < NQ / 2; ++pp) {
            const int qa = 2 * pp, qb = qa + 1;
            // tiles whose products were issued in the previous step get their gradient step
            if (pp >= 1 && pp <= 6) {
                gradient(G[qa + 2], X[qa + 2]);
                gradient(G[qb + 2], X[qb + 2]);
            }
            bf16x8 xf[3];
            if (pp >= 1) split_frag(X[qa - 2], X[qb - 2], xf);
            double w[11];
            int W1[7], W2[7], W3[7];
            float out[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int s = 4 * pp + k, cur = s & 1, nxt = cur ^ 1;
                // MFMAs of this slot's units
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const LnUnit U = ln_unit(pp, k, u);
                    if (U.kind == 1) G[U.a] = split_mfma6(F[cur][u].a, rf[U.b], U.b == 0 ? floatx4{0.f, 0.f, 0.f, 0.f} : G[U.a]);
                    else if (U.kind == 2) R[U.a] = split_mfma6(F[cur][u].a, xf, R[U.a]);
                }
                // operands of the next slot
                const int pn = (k == 3) ? pp + 1 : pp, kn = (k + 1) & 3;
#pragma unroll
                for (int u = 0; u < 2; ++u) ln_load_unit<K>(S, ln_unit(pn, kn, u), AL, F[nxt][u]);
                // NLM phase
                const int q = (k < 2) ? qa : qb;
                if (k == 0 || k == 2) {
                    float prv[3], nx[4];
                    if (q == 0) {
#pragma unroll
                        for (int e = 0; e < 3; ++e) prv[e] = edge_prev[e];
                    } else {
#pragma unroll
                        for (int e = 0; e < 3; ++e) prv[e] = G[q - 1][e + 1];
                    }
                    if (q == NQ - 1) {    // reflect: atoms 256..259 -> 254, 253, 252, 251
                        const float rfl[4] = {G[q][2], G[q][1], G[q][0], G[q - 1][3]};
#pragma unroll
                        for (int e = 0; e < 4; ++e) nx[e] = (g == 3) ? rfl[e] : edge_next[e];
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) nx[e] = G[q + 1][e];
                    }
                    const double wv[11] = {prv[0], prv[1], prv[2], G[q][0], G[q][1], G[q][2], G[q][3],
                                           nx[0], nx[1], nx[2], nx[3]};
#pragma unroll
                    for (int e = 0; e < 11; ++e) w[e] = wv[e];
                    if (q == 0) {
                        nlm_weights<true>(w, kneg, W1, W2, W3);
                    } else {
                        nlm_weights<false>(w, kneg, W1, W2, W3);
                        W1[2] = carry[0];
                        W2[1] = carry[1]; W2[2] = carry[2];
                        W3[0] = carry[3]; W3[1] = carry[4]; W3[2] = carry[5];
                    }
                    carry[0] = W1[6];
                    carry[1] = W2[5]; carry[2] = W2[6];
                    carry[3] = W3[4]; carry[4] = W3[5]; carry[5] = W3[6];
                } else {
                    nlm_outputs<DIV>(w, W1, W2, W3, c0, p.seven, out);
#pragma unroll
                    for (int i = 0; i < 4; ++i) X[q][i] = out[i];
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        {
            bf16x8 xf[3];
            split_frag(X[NQ - 2], X[NQ - 1], xf);
            tm_gemm1<K>(S, NQ / 2 - 1, xf, R, AL);
        }
    }

    if (valid) {
        if (p.coefs) {
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                *reinterpret_cast<float4 *>(&p.coefs[j * K + 64 * g + 4 * q]) =
                    make_float4(X[q][0], X[q][1], X[q][2], X[q][3]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < NT)
                *reinterpret_cast<float4 *>(&p.phi[j * p.n_pad + 16 * t + 4 * g]) =
                    make_float4(R[t][0], R[t][1], R[t][2], R[t][3]);
    }
}

// A second instantiation of k_ista_ln2 (the DIV = 0 quotient, never launched) beside the product's
// <256, 1>: with it the product kernel compiles to exactly round 1's code (30 AGPRs,
// 104 v_accvgpr moves); compiled alone, the same source gets 82 AGPRs and 241 moves, and configs[1]
// loses 2.8 % (k_ista_ln2 7.88 vs 7.59 ms per launch; profiles/r04/ab_pnp).  Every helper is
// __forceinline__, so this is not inlining: the device IR of the product kernel differs in what the
// middle end leaves to the backend (with the second instantiation a dozen [4 x float] / <4 x float>
// allocas survive to AMDGPUPromoteAlloca; alone, SROA splits them earlier), and the register
// allocation of this VGPR-saturated kernel follows.  amdgpu_waves_per_eu, amdgpu_num_vgpr and
// amdgpu_flat_work_group_size on the kernel leave 82.  tests/test_codegen.py reads the built
// library's kernel metadata and fails above 32 AGPRs (or on any spill), so a compiler update or an
// edit here that loses the allocation is caught on the CPU.
template __global__ void k_ista_ln2<256, 0>(IstaParams);

}  // namespace lrs

using namespace lrs;

// k_ista_ln2's quotient: the Newton step on v_rcp_f64 alone.  A further remainder correction
// (nlm_outputs<2>) is also < 1 ulp of fp64 before the float rounding; the register allocation of
// this VGPR-saturated kernel is what differs.
constexpr int kLn2Div = 1;

// The resident kernels (dictionary in LDS) serve n_pad <= 64 with K = 256 and the skimage / soft
// prox; everything else runs the row-split kernel, which needs the fragment-ordered dictionary.
static bool ista_resident(int64_t n_pad, int64_t K, int prox) {
    return n_pad <= kStageRows && K == 256 && prox != LRS_PROX_NLM_MATLAB;
}

// the dense-GEMM path: K > 512, or asked for (lrs_ista_opts.algorithm)
static bool ista_use_generic(int64_t K, const lrs_ista_opts *opts) {
    return K > 512 || (opts && opts->algorithm == LRS_ISTA_ALGO_GENERIC);
}

// FISTA momentum (lrs_ista_opts.accel).  The resident kernels keep the coefficients in VGPRs for all
// of Nit and have no accelerated form: a call with accel at their sizes runs the row-split kernel.
static bool ista_accel(const lrs_ista_opts *opts) { return opts && opts->accel == LRS_ISTA_ACCEL_FISTA; }

extern "C" size_t lrs_ista_workspace(int64_t n, int64_t K, int prox, const lrs_ista_opts *opts) {
    if (n <= 0 || K <= 0) return 0;
    if (ista_use_generic(K, opts)) return ista_generic_workspace(n, K, ista_accel(opts));
    if (ista_resident(round_up(n, 16), K, prox) && !ista_accel(opts)) return 0;
    return ista_rs_workspace(n, K);
}

extern "C" int lrs_ista_f32(const float *Yb, const uint8_t *obs, const float *D, int64_t n,
                            int64_t n_pad, int64_t K, int64_t nb, const float *alpha, const double *thr,
                            int Nit, int prox, float *coefs, float *phi, const lrs_ista_opts *opts, void *ws,
                            size_t ws_bytes, void *stream) {
    if (!Yb || !obs || !D || !alpha || !thr || !phi) return LRS_E_INVALID;
    if (const int rc = ista_check_args(n, n_pad, K, nb, Nit, prox, opts)) return rc;
    if (nb > ((int64_t)1 << 40)) return LRS_E_INVALID;
    if (opts && opts->algorithm != LRS_ISTA_ALGO_AUTO && opts->algorithm != LRS_ISTA_ALGO_GENERIC) return LRS_E_INVALID;
    const int precision = opts ? opts->precision : LRS_ISTA_SPLIT_BF16;   // per call (no process state)
    const int64_t max_wg = opts ? opts->max_workgroups : 0;
    if (nb == 0) return LRS_OK;
    hipStream_t st = (hipStream_t)stream;
    // warm start exists only on the row-split kernel: refuse it before any dispatch (the generic path
    // would otherwise restart from zero on every slice)
    const bool warm = opts && opts->warm_start;
    const bool accel = ista_accel(opts);
    const bool resident = ista_resident(n_pad, K, prox) && !accel;
    if (warm && (!coefs || ista_use_generic(K, opts) || resident)) return LRS_E_UNSUPPORTED;
    if (ista_use_generic(K, opts))
        return ista_generic(Yb, obs, D, n, n_pad, K, nb, alpha, thr, Nit, prox, coefs, phi, ws, ws_bytes, st, accel);
    if (!resident)
        return ista_rs_launch(Yb, obs, D, n, n_pad, K, nb, alpha, thr, Nit, prox, coefs, phi, ws, ws_bytes, max_wg, st,
                              warm ? coefs : nullptr, accel);
    IstaParams p{Yb, obs, D, alpha, thr, coefs, phi, (int)n, (int)n_pad, Nit, prox, nb, 7.0};
    const int64_t blocks_per_wg = (int64_t)kIstaWaves * 16;
    dim3 grid((unsigned)((nb + blocks_per_wg - 1) / blocks_per_wg));
    const bool split = precision == LRS_ISTA_SPLIT_BF16;
    const dim3 grid_b3((unsigned)((nb + kB3Waves * 16 - 1) / (kB3Waves * 16)));
    if (split && prox == LRS_PROX_SOFT)
        hipLaunchKernelGGL((k_ista_b3<256>), grid_b3, dim3(kB3Threads), 0, st, p);
    else if (split)
        hipLaunchKernelGGL((k_ista_ln2<256, kLn2Div>), grid_b3, dim3(kB3Threads), 0, st, p);
    else if (prox == LRS_PROX_SOFT)
        hipLaunchKernelGGL((k_ista_res<256, true>), grid, dim3(kIstaThreads), 0, st, p);
    else
        hipLaunchKernelGGL((k_ista_res<256, false>), grid, dim3(kIstaThreads), 0, st, p);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

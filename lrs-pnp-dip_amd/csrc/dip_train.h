// DIP low-rank prox, the training step around the network: the loss heads (k_masked_mse*, k_mse_head*),
// Adam (k_adam), the step's begin (k_step_begin) and early stopping (k_es_step*, k_es_decide).
// Part of dipnet.hip's translation unit, after dip_kernels.h (block_sum_d1 / block_sum2_d, act_bwd); wt_store
// and agent_add are lrs_common.h's, lrs_es_state is lrspnp.h's.
#pragma once
#include "dip_kernels.h"

namespace lrs {

// ------------------------------------------------------------------------------------------
// Loss: mse(target*mask, out*mask) over C*P (main_LRS_PnP_DIP_1-LiP.py:234); gout = dL/dout.
// mask is null, [P] (mstride 0: broadcast over channels, mask_bkg (1,1,H,W)) or per element [C][P]
// (mstride P: a mask that differs between bands).  norm stays 2 / (C P) in both: MSELoss's mean.
// ------------------------------------------------------------------------------------------
// grid (S, C): workgroup (sb, c) covers pixels [sb*chunk, +chunk) of channel c, so the mask
// index is c * mstride + the pixel (no 64-bit modulo); vec: float4 loads / stores (P, chunk
// multiples of 4; with mstride = P the mask rows are 16-B aligned as those of out and target are).
// (the body of both kernels below; norm = 2 / the element count of the mean)
__device__ __forceinline__ void masked_mse_body(const float *__restrict__ out, const float *__restrict__ target,
                                                const float *__restrict__ mask, int64_t mstride, int64_t P, int chunk,
                                                int vec, float *__restrict__ gout, double *loss_acc, const float norm) {
    __shared__ double red[8];
    const int64_t off = (int64_t)blockIdx.y * P;
    const float *mrow = mask ? mask + (int64_t)blockIdx.y * mstride : nullptr;   // this channel's mask row
    const int64_t i0 = (int64_t)blockIdx.x * chunk, i1 = min(P, i0 + chunk);
    double s = 0.0;
    if (vec) {
        const float4 *o4 = reinterpret_cast<const float4 *>(out + off), *t4 = reinterpret_cast<const float4 *>(target + off);
        const float4 *m4 = reinterpret_cast<const float4 *>(mrow);
        float4 *g4 = gout ? reinterpret_cast<float4 *>(gout + off) : nullptr;
        for (int64_t q = (i0 >> 2) + threadIdx.x; q < (i1 >> 2); q += blockDim.x) {
            const float4 ov = o4[q], tv = t4[q];
            const float4 mv = mask ? m4[q] : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
            const float oe[4] = {ov.x, ov.y, ov.z, ov.w}, te[4] = {tv.x, tv.y, tv.z, tv.w},
                        me[4] = {mv.x, mv.y, mv.z, mv.w};
            float ge[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = te[e] * me[e] - oe[e] * me[e];
                s += (double)d * (double)d;
                ge[e] = (-(norm * d)) * me[e];
            }
            if (g4) g4[q] = make_float4(ge[0], ge[1], ge[2], ge[3]);
        }
    } else {
        for (int64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
            const float mk = mask ? mrow[i] : 1.0f;
            const float a = target[off + i] * mk, b = out[off + i] * mk;
            const float d = a - b;
            s += (double)d * (double)d;
            if (gout) gout[off + i] = (-(norm * d)) * mk;
        }
    }
    s = block_sum_d(s, red);
    if (threadIdx.x == 0) atomicAdd(loss_acc, s);
}

__global__ __launch_bounds__(256) void k_masked_mse(const float *__restrict__ out, const float *__restrict__ target,
                                                    const float *__restrict__ mask, int64_t mstride, int C, int64_t P,
                                                    int chunk, int vec, float *__restrict__ gout, double *loss_acc) {
    masked_mse_body(out, target, mask, mstride, P, chunk, vec, gout, loss_acc, (float)(2.0 / ((double)C * (double)P)));
}

// The same over a framed output: the mask is 0 on the frame, so those elements add nothing to the sum
// and get gout = 0; the mean is over the n_mean interior elements (lrs_dipnet_set_frame) instead of C P.
__global__ __launch_bounds__(256) void k_masked_mse_n(const float *__restrict__ out, const float *__restrict__ target,
                                                      const float *__restrict__ mask, int64_t mstride, int64_t n_mean,
                                                      int64_t P, int chunk, int vec, float *__restrict__ gout,
                                                      double *loss_acc) {
    masked_mse_body(out, target, mask, mstride, P, chunk, vec, gout, loss_acc, (float)(2.0 / (double)n_mean));
}

// Loss head of a training step whose last node is a conv without BN (both reference nets): the
// masked MSE (as k_masked_mse: sum d^2, dL/dout = -(2/(C P)) d m) fused with that node's
// activation backward dL/dz = act'(out) dL/dout and its bias gradient sum_p dL/dz: one pass
// instead of masked-MSE + BN-backward statistics + BN-backward apply.  Grid (S, C), S ~ P / 4096
// (a few thousand workgroups: the pass is HBM-bound only with many loads in flight).  Partials
// (fp64) go to part[c][S] (bias) and part[C S + c][S] (loss); the last workgroup of a channel to
// finish (per-channel counter) sums that channel's partials in order, the last channel to finish
// (counter cnt[C]) sums the channel losses in order into loss_acc: bias gradient and loss are both
// deterministic.  Counters are reset by their last arriver.
__device__ __forceinline__ void mse_head_body(const float *__restrict__ out, const float *__restrict__ target,
                                              const float *__restrict__ mask, int64_t mstride, int C, int64_t P,
                                              int chunk, int vec, int act, float *__restrict__ gz, double *loss_acc,
                                              double *__restrict__ part, int *__restrict__ cnt,
                                              float *__restrict__ gbias, const float norm) {
    __shared__ double red[8];
    __shared__ int last;
    const int c = blockIdx.y, S = gridDim.x;
    const int64_t off = (int64_t)c * P;
    const float *mrow = mask ? mask + (int64_t)c * mstride : nullptr;   // as k_masked_mse: [P] or [C][P]
    const int64_t i0 = (int64_t)blockIdx.x * chunk, i1 = min(P, i0 + chunk);
    double s = 0.0, sb = 0.0;
    if (vec) {
        // one fp64 accumulator pair per float4 lane: four independent dependency chains
        double s4[4] = {0.0, 0.0, 0.0, 0.0}, sb4[4] = {0.0, 0.0, 0.0, 0.0};
        const float4 *o4 = reinterpret_cast<const float4 *>(out + off), *t4 = reinterpret_cast<const float4 *>(target + off);
        const float4 *m4 = reinterpret_cast<const float4 *>(mrow);
        float4 *g4 = reinterpret_cast<float4 *>(gz + off);
        const int q0 = (int)(i0 >> 2), q1 = (int)(i1 >> 2);
        // two float4 per thread per trip: both loads of both in flight together
        for (int q = q0 + threadIdx.x; q < q1; q += 2 * blockDim.x) {
            const bool hb = q + (int)blockDim.x < q1;
            const int qb = hb ? q + (int)blockDim.x : q;   // loads unconditional (all in flight together)
            const float4 ov0 = o4[q], tv0 = t4[q], ov1 = o4[qb], tv1 = t4[qb];
            const float4 one4 = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
            const float4 mv0 = mask ? m4[q] : one4, mv1 = mask ? m4[qb] : one4;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (h == 1 && !hb) break;
                const float4 ov = h ? ov1 : ov0, tv = h ? tv1 : tv0, mv = h ? mv1 : mv0;
                const float oe[4] = {ov.x, ov.y, ov.z, ov.w}, te[4] = {tv.x, tv.y, tv.z, tv.w},
                            me[4] = {mv.x, mv.y, mv.z, mv.w};
                float ge[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float d = te[e] * me[e] - oe[e] * me[e];
                    s4[e] += (double)d * (double)d;
                    ge[e] = act_bwd((-(norm * d)) * me[e], oe[e], act);
                    sb4[e] += (double)ge[e];
                }
                g4[h ? qb : q] = make_float4(ge[0], ge[1], ge[2], ge[3]);
            }
        }
        s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
        sb = (sb4[0] + sb4[1]) + (sb4[2] + sb4[3]);
    } else {
        for (int64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
            const float mk = mask ? mrow[i] : 1.0f;
            const float o = out[off + i];
            const float d = target[off + i] * mk - o * mk;
            s += (double)d * (double)d;
            const float g = act_bwd((-(norm * d)) * mk, o, act);
            gz[off + i] = g;
            sb += (double)g;
        }
    }
    int parity = 0;
    block_sum2_d(s, sb, red);   // (red is free again after the barrier below)
    double *bp = part + (int64_t)c * S, *lp = part + (int64_t)C * S + (int64_t)c * S;
    double *cl = part + 2 * (int64_t)C * S;   // per-channel losses
    // hand-offs without fences (lrs_common.h, wt_store): write-through partials, drain, count
    if (threadIdx.x == 0) {
        wt_store(bp + blockIdx.x, sb);
        wt_store(lp + blockIdx.x, s);
        wt_drain();
        last = agent_add(cnt + c, 1) == S - 1;
    }
    __syncthreads();
    if (!last) return;
    // the channel's partials, summed by the whole workgroup in a fixed tree (S <= 64): deterministic
    const int t = threadIdx.x;
    double tb = t < S ? wt_load(bp + t) : 0.0, tl = t < S ? wt_load(lp + t) : 0.0;
    block_sum2_d(tb, tl, red);
    if (t == 0) {
        gbias[c] = (float)tb;
        agent_store(cnt + c, 0);
        wt_store(cl + c, tl);
        wt_drain();
        last = agent_add(cnt + C, 1) == C - 1;
    }
    __syncthreads();
    if (!last) return;
    double tot = 0.0;
    for (int k = t; k < C; k += blockDim.x) tot += wt_load(cl + k);
    tot = block_sum_d1(tot, red, parity);
    if (t == 0) {
        *loss_acc += tot;
        agent_store(cnt + C, 0);
    }
}

__global__ __launch_bounds__(256) void k_mse_head(const float *__restrict__ out, const float *__restrict__ target,
                                                  const float *__restrict__ mask, int64_t mstride, int C,
                                                  int64_t P, int chunk, int vec, int act,
                                                  float *__restrict__ gz, double *loss_acc,
                                                  double *__restrict__ part, int *__restrict__ cnt,
                                                  float *__restrict__ gbias) {
    mse_head_body(out, target, mask, mstride, C, P, chunk, vec, act, gz, loss_acc, part, cnt, gbias,
                  (float)(2.0 / ((double)C * (double)P)));
}

// the head of a framed output (k_masked_mse_n): the mean over the n_mean interior elements
__global__ __launch_bounds__(256) void k_mse_head_n(const float *__restrict__ out, const float *__restrict__ target,
                                                    const float *__restrict__ mask, int64_t mstride, int C,
                                                    int64_t P, int chunk, int vec, int act,
                                                    float *__restrict__ gz, double *loss_acc,
                                                    double *__restrict__ part, int *__restrict__ cnt,
                                                    float *__restrict__ gbias, int64_t n_mean) {
    mse_head_body(out, target, mask, mstride, C, P, chunk, vec, act, gz, loss_acc, part, cnt, gbias,
                  (float)(2.0 / (double)n_mean));
}

// ------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam defaults: no weight decay, no amsgrad), flat parameter buffer.
// step is a device counter so a captured step replays correctly.
// ------------------------------------------------------------------------------------------
// A weight gradient whose split-K partials Adam itself finishes (the step's last weight gradient,
// lrs_dipnet_train_steps): parameters [beg, beg + len) take g = (sum of the nsplit partials, in
// k_gemm_reduce's order) / *div, which is also stored to the gradient buffer
struct AdamPend {
    const float *part;
    int nsplit;
    int64_t beg, len;
    const float *div;
    float *gout;
};

__device__ __forceinline__ float adam_pend_grad(const AdamPend &a, int64_t idx) {
    const int64_t i = idx - a.beg;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int z = 0;
    for (; z + 8 <= a.nsplit; z += 8)
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] += a.part[(int64_t)(z + u) * a.len + i];
    for (; z < a.nsplit; ++z) acc[z & 7] += a.part[(int64_t)z * a.len + i];
    float s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    if (a.div) s = s / *a.div;
    a.gout[idx] = s;
    return s;
}

__global__ void k_adam(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                       float *__restrict__ v, int64_t n, const int *step, float lr, float b1, float b2,
                       float eps, AdamPend pend) {
    __shared__ float sc[2];   // the bias corrections, once per workgroup (fp64 pow is costly)
    const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
    const int64_t n4 = vec ? n / 4 : 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t q0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // the first float4 of every thread is loaded before thread 0's fp64 pow: the loads' latency and
    // the bias corrections overlap (one float4 per thread covers the whole net at the launch size)
    float4 pv0 = {0.f, 0.f, 0.f, 0.f}, mv0 = pv0, vv0 = pv0, gv0 = pv0;
    if (q0 < n4) {
        pv0 = reinterpret_cast<float4 *>(p)[q0];
        mv0 = reinterpret_cast<float4 *>(m)[q0];
        vv0 = reinterpret_cast<float4 *>(v)[q0];
        gv0 = reinterpret_cast<const float4 *>(g)[q0];
    }
    if (threadIdx.x == 0) {
        const int t = *step;
        const double bc1 = 1.0 - pow((double)b1, (double)t);
        const double bc2 = 1.0 - pow((double)b2, (double)t);
        sc[0] = (float)((double)lr / bc1);
        sc[1] = (float)sqrt(bc2);
    }
    __syncthreads();
    const float step_size = sc[0], bc2s = sc[1];
    // elementwise, so the float4 body (all four buffers 16-B aligned) is bitwise the scalar one
    auto upd = [&](float &pi, float gi, float &mi, float &vi) {
        mi = mi + (1.0f - b1) * (gi - mi);                          // exp_avg.lerp_(grad, 1-b1)
        vi = vi * b2 + (1.0f - b2) * gi * gi;                       // mul_(b2).addcmul_(g, g, 1-b2)
        const float den = sqrtf(vi) / bc2s + eps;
        pi = pi - step_size * (mi / den);
    };
    for (int64_t q = q0; q < n4; q += stride) {
        const bool first = q == q0;
        float4 pv = first ? pv0 : reinterpret_cast<float4 *>(p)[q], mv = first ? mv0 : reinterpret_cast<float4 *>(m)[q],
               vv = first ? vv0 : reinterpret_cast<float4 *>(v)[q];
        float4 gv = first ? gv0 : reinterpret_cast<const float4 *>(g)[q];
        if (pend.part && 4 * q + 3 >= pend.beg && 4 * q < pend.beg + pend.len) {
            if (4 * q >= pend.beg && 4 * q + 3 < pend.beg + pend.len) {
                gv.x = adam_pend_grad(pend, 4 * q); gv.y = adam_pend_grad(pend, 4 * q + 1);
                gv.z = adam_pend_grad(pend, 4 * q + 2); gv.w = adam_pend_grad(pend, 4 * q + 3);
            } else {
                float ge[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * q + e >= pend.beg && 4 * q + e < pend.beg + pend.len) ge[e] = adam_pend_grad(pend, 4 * q + e);
                gv = make_float4(ge[0], ge[1], ge[2], ge[3]);
            }
        }
        upd(pv.x, gv.x, mv.x, vv.x);
        upd(pv.y, gv.y, mv.y, vv.y);
        upd(pv.z, gv.z, mv.z, vv.z);
        upd(pv.w, gv.w, mv.w, vv.w);
        reinterpret_cast<float4 *>(m)[q] = mv;
        reinterpret_cast<float4 *>(v)[q] = vv;
        reinterpret_cast<float4 *>(p)[q] = pv;
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float pi = p[i], mi = m[i], vi = v[i];
        const float gi = (pend.part && i >= pend.beg && i < pend.beg + pend.len) ? adam_pend_grad(pend, i) : g[i];
        upd(pi, gi, mi, vi);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi;
    }
}

__global__ void k_step_begin(double *loss_acc, int *step) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        *loss_acc = 0.0;
        *step += 1;
    }
}

// ------------------------------------------------------------------------------------------
// Early stopping (main_LRS_PnP_DIP_1-LiP.py:71-99, 244-264), on device.
// The reference's metric each step, once the last `size` outputs are collected (myMetric, :102-103):
//   var = mean_j sum_p (ave_p - img_j,p)^2 / N = (Q2 - sum_p A_p^2 / size) / (N size),
// A_p = sum_j img_j,p over the ring and Q2 = sum_p sum_j img_j,p^2, one scalar (the squares' sum needs
// no per-pixel form).  The buffer (lrs_es_ring_bytes) holds the ring [size][N] floats, then A [N]
// (fp64), the per-workgroup partial sums [2][kEsMaxBlocks] and Q2.  One pass per step (k_es_step)
// writes the new output into its slot and slides A (+ new - the slot's old value), so a step reads the
// ring slot it overwrites and nothing else, and its workgroups sum the change of the squares (exact in
// fp64: new^2 - old^2) and A_p^2; k_es_decide adds both in a fixed order (deterministic), slides Q2
// and forms the variance.  Every kEsRefresh windows (the slot of the last index) A and Q2 are
// re-summed from the whole ring in slot order, bounding the sliding sums' rounding drift (~1e-16 per
// update: after 300 updates still ~1e-12 of the variance).  Traffic 28 B per output element per step
// (round 6 first form: 44 B with a per-pixel B_p and a re-sum every window; round 5: the whole ring read
// twice per step -- 1.8 GB per step at 196 x 196 x 198 -- and workgroup sums added with atomics).
// ------------------------------------------------------------------------------------------
constexpr int kEsMaxBlocks = 1024;
constexpr int kEsRefresh = 10;   // windows between re-sums of A and Q2 from the ring

// this output's epoch c (before k_es_decide increments count) re-sums A and Q2 from the ring
__host__ __device__ inline bool es_refresh(int c, int S) { return (c + 1) % (S * kEsRefresh) == 0; }

__host__ __device__ inline int64_t es_ab_offset_bytes(int size, int64_t N) {   // A after the ring, 16-B aligned
    return ((int64_t)size * N * 4 + 15) / 16 * 16;
}

// The interior of a framed output [C][Hf][Wf] as the ring sees it: element i = (c H + y) W + x of the
// [C][H][W] interior lies at (c Hf + top + y) Wf + left + x (lrs_dipnet_set_frame; N <= INT32_MAX).
struct EsCrop {
    int top, left, H, W, Hf, Wf;
};

template <bool kCrop>
__device__ __forceinline__ void es_step_body(const float *__restrict__ out, int64_t N, float *__restrict__ ring,
                                             lrs_es_state *st, const EsCrop cr) {
    __shared__ double red[16];
    const int S = st->size, c = st->count, slot = c % S;   // c: this output's epoch (k_es_decide increments count)
    double *A = reinterpret_cast<double *>(reinterpret_cast<char *>(ring) + es_ab_offset_bytes(S, N));
    double *part = A + N;   // [0 .. kEsMaxBlocks): the squares' change (or sum), then the A^2 sums
    float *dst = ring + (int64_t)slot * N;
    const bool full = c + 1 >= S, refresh = es_refresh(c, S);
    double dq = 0.0, qa = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        float x;
        if (kCrop) {
            const unsigned hw = (unsigned)(cr.H * cr.W), ch = (unsigned)i / hw, r = (unsigned)i - ch * hw;
            const unsigned y = r / (unsigned)cr.W, xx = r - y * (unsigned)cr.W;
            x = out[((int64_t)ch * cr.Hf + cr.top + y) * cr.Wf + cr.left + xx];
        } else {
            x = out[i];
        }
        double a;
        if (refresh) {   // the ring in slot order, the new output in the last slot
            dst[i] = x;
            a = 0.0;
            double q = 0.0;
            for (int j = 0; j < S - 1; ++j) {
                const double v = (double)ring[(int64_t)j * N + i];
                a += v;
                q += v * v;
            }
            a += (double)x;
            q += (double)x * (double)x;
            dq += q;
        } else if (c < S) {   // filling: a plain running sum
            dst[i] = x;
            a = c == 0 ? (double)x : A[i] + (double)x;
            dq += (double)x * (double)x;
        } else {              // sliding: the slot's old output leaves the window
            const float o = dst[i];
            dst[i] = x;
            a = A[i] + ((double)x - (double)o);
            dq += (double)x * (double)x - (double)o * (double)o;
        }
        A[i] = a;
        if (full) qa += a * a;
    }
    block_sum2_d(dq, qa, red);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = dq;
        part[kEsMaxBlocks + blockIdx.x] = qa;
    }
}

__global__ __launch_bounds__(256) void k_es_step(const float *__restrict__ out, int64_t N, float *__restrict__ ring,
                                                lrs_es_state *st) {
    es_step_body<false>(out, N, ring, st, EsCrop{});
}

// the same update fed the interior of a framed output: the ring, the window sums and the variance test
// are those of the cropped [C][H][W] image (same workgroups, same order: bit-identical to k_es_step on a crop)
__global__ __launch_bounds__(256) void k_es_step_crop(const float *__restrict__ out, int64_t N, float *__restrict__ ring,
                                                     lrs_es_state *st, EsCrop cr) {
    es_step_body<true>(out, N, ring, st, cr);
}

// one wave: the nblk partials of k_es_step in a fixed order, then the reference's patience test
__global__ void k_es_decide(const float *ring, int64_t N, int nblk, lrs_es_state *st) {
    const int S = st->size;
    double *part = reinterpret_cast<double *>(reinterpret_cast<char *>(const_cast<float *>(ring)) + es_ab_offset_bytes(S, N)) + N;
    double *q2 = part + 2 * kEsMaxBlocks;   // the window's sum of squares
    double dq = 0.0, qa = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 64) {
        dq += part[b];
        qa += part[kEsMaxBlocks + b];
    }
    dq = wave_sum_butterfly(dq);   // fixed order
    qa = wave_sum_butterfly(qa);
    if (threadIdx.x != 0) return;
    const int epoch = st->count;           // iteration index i of the reference loop
    const double q = (epoch == 0 || es_refresh(epoch, S)) ? dq : *q2 + dq;
    *q2 = q;
    const double v = q - qa / (double)S;
    st->count += 1;
    if (st->count >= S && !st->stop) {
        const double var = v / (double)N / (double)S;
        st->last_var = var;
        if (var < st->best) {
            st->best = var;
            st->best_epoch = epoch;
            st->wait = 0;
        } else {
            st->wait += 1;
            if (st->wait >= st->patience) {
                st->stop = 1;
                st->stop_epoch = epoch;
            }
        }
    }
}

}  // namespace lrs

namespace {   // (internal linkage: this header is part of dipnet.hip's translation unit only)

__global__ void k_es_init(lrs_es_state *st, int size, int patience) {
    st->count = 0;
    st->size = size;
    st->patience = patience;
    st->wait = 0;
    st->stop = 0;
    st->stop_epoch = -1;
    st->best_epoch = 0;
    st->reserved = 0;
    st->best = INFINITY;
    st->var_acc = 0.0;
    st->last_var = NAN;
}

}  // namespace

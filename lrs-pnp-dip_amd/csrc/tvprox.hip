// TV low-rank-slot prox on the unfolded cube (lrs_tvprox_f32):
//   U = argmin_u 1/2 ||u - Z||^2 + tau T(u),  Z = fl(X + fl(c2 L2)),
//   T(u) = w_sp sum(|Dy u| + |Dx u|) + w_bd sum |Dc u| + w_ss sum(|Dy Dc u| + |Dx Dc u|),
// the operators, their association and their index sets those of lrs_sstv_f32 (dip_tv.h), by the fast
// gradient projection on the dual (Beck-Teboulle FGP) with a fixed iteration count, in fp32.
//
// Layout: X, L2, U are [P][B], p = i + H j, the image o[c = b][y = i][x = j]: Dc runs along the contiguous
// axis, Dy has stride B and Dx stride H B.  K stacks the five difference fields y, x, c, yc, xc; a field is
// a cube-sized array in ws that holds its dual value at the difference's lowest-index element and 0 where
// the difference does not exist (the last row / column / band), so the adjoint needs a guard only where a
// neighbour would leave the row, the column or the pixel.  A field whose weight is 0 or whose index set is
// empty (a dimension of 1) has no array traffic at all.
//
// Per iteration two launches, the launch boundary the only grid-wide synchronisation:
//   k_tvp_primal  u = Z - K^T q      a gather of 14 field values per element in a fixed order (no atomics)
//   k_tvp_dual    p = clip(q + K u / L, -r, r),  q = p + beta (p - p_old)     in place, own element only
// and one more k_tvp_primal on p writes U.  u and q are stored (DESIGN.md §12 weighs the alternatives).
// The first iteration of a cold call has q = p_old = 0 and u = Z: its primal pass is skipped and its dual
// pass forms Z at the stencil points from X and L2, so ws is never read before it is written.  The first
// iteration of a warm call reads the p the last call left, clipped to the current radii, as q and p_old.
//
// A thread owns V consecutive bands of one pixel: V = 4 (16-byte loads and stores) when B % 4 == 0 and
// every base is 16-byte aligned, V = 2 when B % 2 == 0 and the bases are 8-byte aligned (198 bands), else
// V = 1.  An element's arithmetic does not depend on V: the three forms give the same bits.
#include <math.h>

#include <algorithm>

#include "lrs_common.h"

using namespace lrs;

namespace {

constexpr int kTvpThreads = 256;
constexpr int kTvpStatWgs = 1024;   // workgroups (and fp64 partial pairs) of the stats pass at most
enum { kFy = 0, kFx, kFc, kFyc, kFxc, kFields };
enum { kStartNone = 0, kStartCold = 1, kStartWarm = 2 };

struct TvpFields {
    float *f[kFields];   // null: the field is inactive
};

struct TvpArgs {
    const float *X, *L2;
    float c2;
    int H, W, B;
    unsigned strips, items;   // B / V; P * strips
    float r[kFields];         // box radii tau w, rounded once to fp32
};

template <int V> struct VecOf;
template <> struct VecOf<1> { typedef float type; };
template <> struct VecOf<2> { typedef float2 type; };
template <> struct VecOf<4> { typedef float4 type; };

template <int V>
__device__ __forceinline__ void ldv(const float *p, float *v) {
    const typename VecOf<V>::type t = *reinterpret_cast<const typename VecOf<V>::type *>(p);
    const float *s = reinterpret_cast<const float *>(&t);
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = s[k];
}
template <int V>
__device__ __forceinline__ void stv(float *p, const float *v) {
    typename VecOf<V>::type t;
    float *s = reinterpret_cast<float *>(&t);
#pragma unroll
    for (int k = 0; k < V; ++k) s[k] = v[k];
    *reinterpret_cast<typename VecOf<V>::type *>(p) = t;
}

__device__ __forceinline__ float tvp_clip(float v, float r) { return fminf(fmaxf(v, -r), r); }

// Z at `at`: fl(X + fl(c2 L2)) (-ffp-contract=off: two roundings, as torch's X + c2 * L2)
__device__ __forceinline__ float tvp_z(const TvpArgs &a, int64_t at) {
    return a.L2 ? a.X[at] + a.c2 * a.L2[at] : a.X[at];
}
template <int V>
__device__ __forceinline__ void tvp_zv(const TvpArgs &a, int64_t at, float *v) {
    ldv<V>(a.X + at, v);
    if (a.L2) {
        float l[V];
        ldv<V>(a.L2 + at, l);
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = v[k] + a.c2 * l[k];
    }
}

// v[1 .. V] = f[at .. at + V) and v[0] = f[at - 1], 0 where `row` / `left` say the operand is outside;
// clip: the values clipped to +-r (a warm call's first read of p)
template <int V>
__device__ __forceinline__ void tvp_field_row(const float *f, int64_t at, bool row, bool left, bool clip, float r,
                                              float *v) {
#pragma unroll
    for (int k = 0; k <= V; ++k) v[k] = 0.0f;
    if (!row) return;
    ldv<V>(f + at, v + 1);
    if (left) v[0] = f[at - 1];
    if (clip) {
#pragma unroll
        for (int k = 0; k <= V; ++k) v[k] = tvp_clip(v[k], r);
    }
}

struct TvpAt {
    int i, j, b0;
    int64_t at;
};
__device__ __forceinline__ TvpAt tvp_at(const TvpArgs &a, unsigned it, int V) {
    const unsigned s = it % a.strips, pix = it / a.strips;
    TvpAt t;
    t.i = (int)(pix % (unsigned)a.H);
    t.j = (int)(pix / (unsigned)a.H);
    t.b0 = (int)s * V;
    t.at = (int64_t)pix * a.B + t.b0;
    return t;
}

// out = Z - K^T q (q: the fields given).  acc = (((ty + tx) + tc) + tyc) + txc over the active fields,
//   ty = q_y[i-1] - q_y[i], tx likewise, tc = q_c[b-1] - q_c[b],
//   tyc = g(b-1) - g(b) with g(b) = q_yc[b, i-1] - q_yc[b, i], txc likewise along j.
template <int V>
__global__ __launch_bounds__(kTvpThreads) void k_tvp_primal(const TvpArgs a, const TvpFields q, const int clip,
                                                            float *__restrict__ out) {
    const unsigned it = blockIdx.x * (unsigned)kTvpThreads + threadIdx.x;
    if (it >= a.items) return;
    const TvpAt t = tvp_at(a, it, V);
    const int64_t sy = a.B, sx = (int64_t)a.H * a.B;
    const bool up = t.i > 0, lf = t.j > 0, lo = t.b0 > 0;
    float z[V], acc[V];
    tvp_zv<V>(a, t.at, z);
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.0f;
    float cur[V + 1], prv[V + 1];
    if (q.f[kFy]) {
        tvp_field_row<V>(q.f[kFy], t.at, true, false, clip, a.r[kFy], cur);
        tvp_field_row<V>(q.f[kFy], t.at - sy, up, false, clip, a.r[kFy], prv);
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] += prv[k + 1] - cur[k + 1];
    }
    if (q.f[kFx]) {
        tvp_field_row<V>(q.f[kFx], t.at, true, false, clip, a.r[kFx], cur);
        tvp_field_row<V>(q.f[kFx], t.at - sx, lf, false, clip, a.r[kFx], prv);
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] += prv[k + 1] - cur[k + 1];
    }
    if (q.f[kFc]) {
        tvp_field_row<V>(q.f[kFc], t.at, true, lo, clip, a.r[kFc], cur);
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] += cur[k] - cur[k + 1];
    }
    if (q.f[kFyc]) {
        tvp_field_row<V>(q.f[kFyc], t.at, true, lo, clip, a.r[kFyc], cur);
        tvp_field_row<V>(q.f[kFyc], t.at - sy, up, lo, clip, a.r[kFyc], prv);
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] += (prv[k] - cur[k]) - (prv[k + 1] - cur[k + 1]);
    }
    if (q.f[kFxc]) {
        tvp_field_row<V>(q.f[kFxc], t.at, true, lo, clip, a.r[kFxc], cur);
        tvp_field_row<V>(q.f[kFxc], t.at - sx, lf, lo, clip, a.r[kFxc], prv);
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] += (prv[k] - cur[k]) - (prv[k + 1] - cur[k + 1]);
    }
#pragma unroll
    for (int k = 0; k < V; ++k) z[k] = z[k] - acc[k];
    stv<V>(out + t.at, z);
}

// v[0 .. V) = u[at .. at + V) and v[V] = u[at + V], 0 where `row` / `right` say the operand is outside;
// cold: u is Z, formed from X and L2
template <int V>
__device__ __forceinline__ void tvp_u_row(const TvpArgs &a, const float *u, bool cold, int64_t at, bool row,
                                          bool right, float *v) {
#pragma unroll
    for (int k = 0; k <= V; ++k) v[k] = 0.0f;
    if (!row) return;
    if (cold) {
        tvp_zv<V>(a, at, v);
        if (right) v[V] = tvp_z(a, at + V);
    } else {
        ldv<V>(u + at, v);
        if (right) v[V] = u[at + V];
    }
}

// One field's dual update at the thread's V elements: d = (K u) there, ok[k] = the difference exists
template <int V>
__device__ __forceinline__ void tvp_dual_field(float *pf, float *qf, int64_t at, int start, float r, float invL,
                                               float beta, const float *d, const bool *ok) {
    float qv[V], po[V], pn[V], qn[V];
    if (start == kStartNone) {
        ldv<V>(qf + at, qv);
        ldv<V>(pf + at, po);
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) qv[k] = 0.0f;
        if (start == kStartWarm) {
            ldv<V>(pf + at, qv);
#pragma unroll
            for (int k = 0; k < V; ++k) qv[k] = tvp_clip(qv[k], r);
        }
#pragma unroll
        for (int k = 0; k < V; ++k) po[k] = qv[k];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
        pn[k] = ok[k] ? tvp_clip(qv[k] + invL * d[k], r) : 0.0f;
        qn[k] = ok[k] ? pn[k] + beta * (pn[k] - po[k]) : 0.0f;
    }
    stv<V>(pf + at, pn);
    stv<V>(qf + at, qn);
}

template <int V>
__global__ __launch_bounds__(kTvpThreads) void k_tvp_dual(const TvpArgs a, const TvpFields p, const TvpFields q,
                                                          const float *__restrict__ u, const int start,
                                                          const float invL, const float beta) {
    const unsigned it = blockIdx.x * (unsigned)kTvpThreads + threadIdx.x;
    if (it >= a.items) return;
    const TvpAt t = tvp_at(a, it, V);
    const int64_t sy = a.B, sx = (int64_t)a.H * a.B;
    const bool dn = t.i + 1 < a.H, rt = t.j + 1 < a.W, hi = t.b0 + V < a.B;
    const bool cold = start == kStartCold;
    const bool bands = p.f[kFc] || p.f[kFyc] || p.f[kFxc];
    float c0[V + 1], cy[V + 1], cx[V + 1], d[V];
    bool ok[V], okb[V];
    tvp_u_row<V>(a, u, cold, t.at, true, hi && bands, c0);
    tvp_u_row<V>(a, u, cold, t.at + sy, dn && (p.f[kFy] || p.f[kFyc]), hi && p.f[kFyc], cy);
    tvp_u_row<V>(a, u, cold, t.at + sx, rt && (p.f[kFx] || p.f[kFxc]), hi && p.f[kFxc], cx);
#pragma unroll
    for (int k = 0; k < V; ++k) okb[k] = k + 1 < V || hi;
    if (p.f[kFy]) {
#pragma unroll
        for (int k = 0; k < V; ++k) { d[k] = cy[k] - c0[k]; ok[k] = dn; }
        tvp_dual_field<V>(p.f[kFy], q.f[kFy], t.at, start, a.r[kFy], invL, beta, d, ok);
    }
    if (p.f[kFx]) {
#pragma unroll
        for (int k = 0; k < V; ++k) { d[k] = cx[k] - c0[k]; ok[k] = rt; }
        tvp_dual_field<V>(p.f[kFx], q.f[kFx], t.at, start, a.r[kFx], invL, beta, d, ok);
    }
    if (p.f[kFc]) {
#pragma unroll
        for (int k = 0; k < V; ++k) d[k] = c0[k + 1] - c0[k];
        tvp_dual_field<V>(p.f[kFc], q.f[kFc], t.at, start, a.r[kFc], invL, beta, d, okb);
    }
    if (p.f[kFyc]) {
#pragma unroll
        for (int k = 0; k < V; ++k) { d[k] = (cy[k + 1] - cy[k]) - (c0[k + 1] - c0[k]); ok[k] = dn && okb[k]; }
        tvp_dual_field<V>(p.f[kFyc], q.f[kFyc], t.at, start, a.r[kFyc], invL, beta, d, ok);
    }
    if (p.f[kFxc]) {
#pragma unroll
        for (int k = 0; k < V; ++k) { d[k] = (cx[k + 1] - cx[k]) - (c0[k + 1] - c0[k]); ok[k] = rt && okb[k]; }
        tvp_dual_field<V>(p.f[kFxc], q.f[kFxc], t.at, start, a.r[kFxc], invL, beta, d, ok);
    }
}

// The workgroup's sum in a fixed order: the waves' butterfly sums, added in wave order
__device__ __forceinline__ double tvp_block_sum(double v, double *red) {
    const double w = wave_sum_butterfly(v);
    __syncthreads();   // (red may still be read from the previous call)
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = w;
    __syncthreads();
    double s = 0.0;
    for (int k = 0; k < kTvpThreads / kWave; ++k) s += red[k];
    return s;
}

// The returned pair's primal objective and duality gap, as per-workgroup fp64 partials (part[2 g], [2 g + 1]):
//   obj = 1/2 sum (U - Z)^2 + sum_f tw_f |K_f U|,   gap = sum_f (r_f |K_f U| - p_f K_f U),
// tw = tau w in fp64, r = the fp32 radius the iteration clipped to (so every term of the gap is >= 0);
// the differences of U are taken in fp64.  p null in every field given: p = 0.
__global__ __launch_bounds__(kTvpThreads) void k_tvp_stats(const TvpArgs a, const TvpFields p, const unsigned active,
                                                           const double tw_y, const double tw_x, const double tw_c,
                                                           const double tw_yc, const double tw_xc,
                                                           const float *__restrict__ U, const unsigned n,
                                                           double *__restrict__ part) {
    __shared__ double red[kTvpThreads / kWave];
    const double tw[kFields] = {tw_y, tw_x, tw_c, tw_yc, tw_xc};
    const int64_t sy = a.B, sx = (int64_t)a.H * a.B;
    double obj = 0.0, gap = 0.0;
    for (unsigned e = blockIdx.x * (unsigned)kTvpThreads + threadIdx.x; e < n; e += gridDim.x * (unsigned)kTvpThreads) {
        const unsigned pix = e / (unsigned)a.B;
        const int b = (int)(e % (unsigned)a.B), i = (int)(pix % (unsigned)a.H), j = (int)(pix / (unsigned)a.H);
        const bool dn = i + 1 < a.H, rt = j + 1 < a.W, hi = b + 1 < a.B;
        const double u0 = (double)U[e], dz = u0 - (double)tvp_z(a, e);
        obj += 0.5 * dz * dz;
        const double ub = hi ? (double)U[e + 1] : 0.0;
        const double uy = dn ? (double)U[e + sy] : 0.0, uyb = dn && hi ? (double)U[e + sy + 1] : 0.0;
        const double ux = rt ? (double)U[e + sx] : 0.0, uxb = rt && hi ? (double)U[e + sx + 1] : 0.0;
        const double d[kFields] = {uy - u0, ux - u0, ub - u0, (uyb - uy) - (ub - u0), (uxb - ux) - (ub - u0)};
        const bool ok[kFields] = {dn, rt, hi, dn && hi, rt && hi};
#pragma unroll
        for (int f = 0; f < kFields; ++f) {
            if (!(active >> f & 1u) || !ok[f]) continue;
            const double ad = fabs(d[f]);
            obj += tw[f] * ad;
            gap += (double)a.r[f] * ad - (p.f[f] ? (double)p.f[f][e] * d[f] : 0.0);
        }
    }
    const double so = tvp_block_sum(obj, red), sg = tvp_block_sum(gap, red);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = so;
        part[2 * blockIdx.x + 1] = sg;
    }
}

// stats[0], stats[1] = the partials' sums, one workgroup, a fixed order
__global__ __launch_bounds__(kTvpThreads) void k_tvp_stats_reduce(const double *__restrict__ part, const int nwg,
                                                                  double *__restrict__ stats) {
    __shared__ double red[kTvpThreads / kWave];
    double so = 0.0, sg = 0.0;
    for (int g = threadIdx.x; g < nwg; g += kTvpThreads) {
        so += part[2 * g];
        sg += part[2 * g + 1];
    }
    so = tvp_block_sum(so, red);
    sg = tvp_block_sum(sg, red);
    if (threadIdx.x == 0) {
        stats[0] = so;
        stats[1] = sg;
    }
}

// H W B when every size is positive and the product is below 2^31, else 0 (bad sizes) or -1 (too large)
int64_t tvp_count(int64_t H, int64_t W, int64_t B) {
    if (H <= 0 || W <= 0 || B <= 0) return 0;
    const int64_t lim = (int64_t)1 << 31;
    if (H >= lim || W >= lim || B >= lim || H * W >= lim || H * W * B >= lim) return -1;
    return H * W * B;
}

// ws: u, p[5], q[5] (each n4 = N rounded up to 4 floats, so every array is 16-byte aligned when ws is), then
// the stats partials; p's arrays keep their places whatever is active (LRS_TVPROX_WARM finds them)
struct TvpWs {
    float *u;
    TvpFields p, q;
    double *part;
};
size_t tvp_ws_bytes(int64_t n) { return (size_t)round_up(n, 4) * 4 * (1 + 2 * kFields) + sizeof(double) * 2 * kTvpStatWgs; }
TvpWs tvp_ws_layout(void *ws, int64_t n, unsigned active) {
    const int64_t n4 = round_up(n, 4);
    float *base = (float *)ws;
    TvpWs w;
    w.u = base;
    for (int f = 0; f < kFields; ++f) {
        const bool on = active >> f & 1u;
        w.p.f[f] = on ? base + (1 + f) * n4 : nullptr;
        w.q.f[f] = on ? base + (1 + kFields + f) * n4 : nullptr;
    }
    w.part = (double *)(base + (1 + 2 * kFields) * n4);
    return w;
}

template <int V>
int tvp_run(TvpArgs a, const TvpWs &w, int n_iter, bool warm, float invL, float *U, hipStream_t st) {
    a.strips = (unsigned)(a.B / V);
    a.items = (unsigned)((int64_t)a.H * a.W * a.strips);
    const dim3 grid((a.items + kTvpThreads - 1) / kTvpThreads), block(kTvpThreads);
    const TvpFields none{};
    double tk = 1.0;   // t_k; beta_1 = 0
    for (int k = 1; k <= n_iter; ++k) {
        const int start = k > 1 ? kStartNone : warm ? kStartWarm : kStartCold;
        if (start != kStartCold) {
            hipLaunchKernelGGL(k_tvp_primal<V>, grid, block, 0, st, a, start == kStartWarm ? w.p : w.q,
                               start == kStartWarm ? 1 : 0, w.u);
            LRS_CHECK_LAUNCH();
        }
        const double tn = 0.5 * (1.0 + sqrt(1.0 + 4.0 * tk * tk));
        const float beta = (float)((tk - 1.0) / tn);
        tk = tn;
        hipLaunchKernelGGL(k_tvp_dual<V>, grid, block, 0, st, a, w.p, w.q, w.u, start, invL, beta);
        LRS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_tvp_primal<V>, grid, block, 0, st, a, n_iter > 0 ? w.p : none, 0, U);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

inline bool tvp_aligned(const void *p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

}  // namespace

extern "C" size_t lrs_tvprox_workspace(int64_t H, int64_t W, int64_t B) {
    const int64_t n = tvp_count(H, W, B);
    return n > 0 ? tvp_ws_bytes(n) : 0;
}

extern "C" int lrs_tvprox_f32(const float *X, const float *L2, float c2, int64_t H, int64_t W, int64_t B, float w_sp,
                              float w_bd, float w_ss, double tau, int n_iter, int flags, float *U, double *stats,
                              void *ws, size_t ws_bytes, void *stream) {
    if (!X || !U || !ws || H <= 0 || W <= 0 || B <= 0 || !(w_sp >= 0.0f) || !(w_bd >= 0.0f) || !(w_ss >= 0.0f) ||
        !(tau >= 0.0) || n_iter < 0 || (flags & ~LRS_TVPROX_WARM))
        return LRS_E_INVALID;
    const int64_t n = tvp_count(H, W, B);
    if (n < 0) return LRS_E_UNSUPPORTED;
    if (ws_bytes < tvp_ws_bytes(n)) return LRS_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const float wf[kFields] = {w_sp, w_sp, w_bd, w_ss, w_ss};
    const bool some[kFields] = {H > 1, W > 1, B > 1, H > 1 && B > 1, W > 1 && B > 1};
    TvpArgs a{X, L2, c2, (int)H, (int)W, (int)B, 0, 0, {}};
    // all weights 0, tau = 0 or n_iter = 0: U = Z, by the primal pass without a field
    const bool solve = tau > 0.0 && n_iter > 0;
    unsigned active = 0;
    double tw[kFields];
    for (int f = 0; f < kFields; ++f) {
        tw[f] = tau * (double)wf[f];
        a.r[f] = (float)tw[f];
        if (wf[f] > 0.0f && tau > 0.0 && some[f]) active |= 1u << f;
    }
    const float invL = 1.0f / (8.0f * (w_sp > 0.0f) + 4.0f * (w_bd > 0.0f) + 32.0f * (w_ss > 0.0f));
    const TvpWs w = tvp_ws_layout(ws, n, active);
    const int iters = solve && active ? n_iter : 0;
    const bool warm = flags & LRS_TVPROX_WARM;
    const bool al16 = tvp_aligned(X, 16) && tvp_aligned(L2, 16) && tvp_aligned(U, 16) && tvp_aligned(ws, 16);
    const bool al8 = tvp_aligned(X, 8) && tvp_aligned(L2, 8) && tvp_aligned(U, 8) && tvp_aligned(ws, 16);
    int rc;
    if (B % 4 == 0 && al16) rc = tvp_run<4>(a, w, iters, warm, invL, U, st);
    else if (B % 2 == 0 && al8) rc = tvp_run<2>(a, w, iters, warm, invL, U, st);
    else rc = tvp_run<1>(a, w, iters, warm, invL, U, st);
    if (rc != LRS_OK || !stats) return rc;
    // n_iter = 0: the pair (Z, p = 0), whose objective is tau T(Z) and whose gap is the same sum
    const int nwg = (int)std::min<int64_t>((n + kTvpThreads - 1) / kTvpThreads, kTvpStatWgs);
    hipLaunchKernelGGL(k_tvp_stats, dim3(nwg), dim3(kTvpThreads), 0, st, a, iters > 0 ? w.p : TvpFields{}, active,
                       tw[kFy], tw[kFx], tw[kFc], tw[kFyc], tw[kFxc], U, (unsigned)n, w.part);
    LRS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_tvp_stats_reduce, dim3(1), dim3(kTvpThreads), 0, st, w.part, nwg, stats);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

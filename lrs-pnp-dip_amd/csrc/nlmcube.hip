// Spectral non-local-means prox on the unfolded cube (lrs_nlmcube_f32): one weight per pixel
// pair, computed from all bands, applied to every band.  With Z = fl(X + fl(c2 L2)), rp = patch_size / 2,
// rs = patch_distance, m() the reflection without edge repeat continued periodically:
//   d(e, e') = sum_c (z[c, m(e)] - z[c, m(e')])^2               pixel distance on extended coordinates
//   D(p, t)  = sum_{|dy|, |dx| <= rp} d(p + delta, p + delta + t)  patch distance
//   w(p, t)  = exp(-max(D / (B (2 rp + 1)^2) - s2, 0) ih2)        for |ty|, |tx| <= rs with p + t inside the image
//   U[c, p]  = sum_t w(p, t) z[c, p + t] / sum_t w(p, t)
//
// Layout: X, L2, U are [P][B], p = y + H x: a pixel's spectrum is contiguous, so a spatial tile and its halo
// load as whole coalesced rows with no layout transform.
//
// One launch, no workspace.  A workgroup owns an 8 x 8 tile; everything between the two passes over the
// spectra lives in LDS:
//   A  the halo (tile +- (rp + rs)) streams through LDS in chunks of cb bands; a thread owns one extended
//      position e of tile +- rp and one row ty of offsets and adds this chunk's share of d(e, e + t) for the
//      2 rs + 1 offsets of that row: fp32, bands in ascending order within a chunk, chunks in ascending order
//   B  D = the (2 rp + 1)^2 box sum of d in fp64, the weight in fp64, rounded once to fp32; 0 where the
//      candidate is outside the image
//   C  the halo tile +- rs streams through LDS again; a thread owns one pixel and every fourth band of the
//      chunk and sums w z over the offsets (ty outer, tx inner) in fp64; U = (float)(sum / sum_t w), staged
//      through LDS so that the stores are whole coalesced rows too
// Nothing is shared between workgroups and every sum has a fixed order: no atomics, reruns are bit-identical.
//
// A thread loads and stores V consecutive bands: V = 4 (16-byte accesses) when B % 4 == 0 and every base is
// 16-byte aligned, V = 2 when B % 2 == 0 and the bases are 8-byte aligned (198 bands), else V = 1.  V shapes
// the global accesses only: the chunk length depends on (rp, rs) alone and the LDS image is the same, so the
// three forms give the same bits.
#include <math.h>

#include "lrs_common.h"

using namespace lrs;

namespace {

constexpr int kNlmThreads = 256;
constexpr int kNlmTile = 8;                       // tile edge: 64 pixels, one wave per band lane in phase C
constexpr int kNlmPix = kNlmTile * kNlmTile;
constexpr int kNlmMaxRp = 3, kNlmMaxRs = 5;
constexpr int kNlmMaxNt = 2 * kNlmMaxRs + 1;      // offsets per row of the search window
constexpr int kNlmMaxChunk = 32;                  // bands per chunk at most
constexpr int kNlmBandLanes = kNlmThreads / kNlmPix;
constexpr size_t kNlmLds = 160 * 1024;
constexpr int kNlmInFlight = 8;                   // pieces a thread loads before it uses the first

struct NlmArgs {
    const float *X, *L2;
    float c2;
    float *U;
    int H, W, B;
    int rp, rs;
    int cb, lcb;       // bands per chunk (8, 16 or 32) and its log2
    int tiles_y;
    double ih2, s2;    // the fp32-rounded 1 / h^2 and 2 sigma^2, widened
    double n;          // B (2 rp + 1)^2
};

template <int V> struct NlmVec;
template <> struct NlmVec<1> { typedef float type; static constexpr int log2 = 0; };
template <> struct NlmVec<2> { typedef float2 type; static constexpr int log2 = 1; };
template <> struct NlmVec<4> { typedef float4 type; static constexpr int log2 = 2; };

// m(e) on an axis of length n
__device__ __forceinline__ int nlm_reflect(int64_t e, int n) {
    if (n == 1) return 0;
    const int64_t per = 2 * ((int64_t)n - 1);
    int64_t r = e % per;
    if (r < 0) r += per;
    return (int)(r < n ? r : per - r);
}

// zs[k][0 .. cb) = Z[pix[k]][c0 .. c0 + cb) for the halo positions k = ey + E ex, ey, ex in [lo, lo + side);
// consecutive threads take consecutive V-band pieces of one spectrum
template <int V>
__device__ __forceinline__ void nlm_load(const NlmArgs &a, const int *pix, float *zs, int E, int S, int lo, int side,
                                         int c0, int cb) {
    typedef typename NlmVec<V>::type vec;
    const int lv = a.lcb - NlmVec<V>::log2;
    const int items = (side * side) << lv;
    // kNlmInFlight pieces per thread are requested before the first is used: the loads' latency overlaps
    for (int base = threadIdx.x; base < items; base += kNlmInFlight * kNlmThreads) {
        vec x[kNlmInFlight], l[kNlmInFlight];
        int to[kNlmInFlight];   // where the piece goes in zs; -1: none
#pragma unroll
        for (int u = 0; u < kNlmInFlight; ++u) {
            const int it = base + u * kNlmThreads;
            const int c = (it & ((1 << lv) - 1)) * V, r = it >> lv;
            to[u] = -1;
            if (it >= items || c >= cb) continue;
            const int k = (lo + r % side) + E * (lo + r / side);
            const int64_t at = (int64_t)pix[k] * a.B + c0 + c;
            to[u] = k * S + c;
            x[u] = *reinterpret_cast<const vec *>(a.X + at);
            if (a.L2) l[u] = *reinterpret_cast<const vec *>(a.L2 + at);
        }
#pragma unroll
        for (int u = 0; u < kNlmInFlight; ++u) {
            if (to[u] < 0) continue;
            const float *xs = reinterpret_cast<const float *>(&x[u]), *ls = reinterpret_cast<const float *>(&l[u]);
            // fl(X + fl(c2 L2)) (-ffp-contract=off: two roundings, as torch's X + c2 * L2)
#pragma unroll
            for (int j = 0; j < V; ++j) zs[to[u] + j] = a.L2 ? xs[j] + a.c2 * ls[j] : xs[j];
        }
    }
}

template <int V>
__global__ __launch_bounds__(kNlmThreads) void k_nlmcube(const NlmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float nlm_lds[];
    const int rp = a.rp, rs = a.rs, nt = 2 * rs + 1, T = nt * nt;
    const int PH = kNlmTile + 2 * rp, NPOS = PH * PH;   // extended positions whose d the tile's patches need
    const int E = kNlmTile + 2 * (rp + rs);             // halo edge
    const int S = a.cb + 1;                             // odd row stride: pixels a lane apart fall on different banks
    float *dacc = nlm_lds;                  // [NPOS][T]   d(e, e + t)
    float *wts = dacc + NPOS * T;           // [64][T]     w(p, t)
    float *outs = wts + kNlmPix * T;        // [64][S]     a chunk of U before it is stored
    float *zs = outs + kNlmPix * S;         // [E E][S]    a chunk of the halo's spectra
    int *pix = (int *)(zs + E * E * S);     // [E E]       the image pixel m(e) of every halo position
    const int tid = threadIdx.x;
    const int64_t y0 = (int64_t)(blockIdx.x % (unsigned)a.tiles_y) * kNlmTile;
    const int64_t x0 = (int64_t)(blockIdx.x / (unsigned)a.tiles_y) * kNlmTile;

    for (int k = tid; k < E * E; k += kNlmThreads)
        pix[k] = nlm_reflect(y0 - (rp + rs) + k % E, a.H) + a.H * nlm_reflect(x0 - (rp + rs) + k / E, a.W);
    __syncthreads();

    // ---- A: pixel distances ------------------------------------------------------------------------
    for (int c0 = 0; c0 < a.B; c0 += a.cb) {
        const int cb = min(a.cb, a.B - c0);
        nlm_load<V>(a, pix, zs, E, S, 0, E, c0, cb);
        __syncthreads();
        for (int item = tid; item < NPOS * nt; item += kNlmThreads) {
            const int pos = item % NPOS, tyi = item / NPOS;
            const int ke = (pos % PH + rs) + E * (pos / PH + rs);   // e = tile - rp + (py, px) in halo coordinates
            const float *za = zs + ke * S;
            const float *zb = zs + (ke + (tyi - rs) - E * rs) * S;  // e + (ty, -rs)
            float acc[kNlmMaxNt];
#pragma unroll
            for (int k = 0; k < kNlmMaxNt; ++k) acc[k] = 0.0f;
            for (int c = 0; c < cb; ++c) {
                const float ze = za[c];
#pragma unroll
                for (int k = 0; k < kNlmMaxNt; ++k)
                    if (k < nt) {
                        const float df = ze - zb[k * E * S + c];
                        acc[k] = fmaf(df, df, acc[k]);
                    }
            }
            float *d = dacc + pos * T + tyi * nt;
#pragma unroll
            for (int k = 0; k < kNlmMaxNt; ++k)
                if (k < nt) d[k] = c0 ? d[k] + acc[k] : acc[k];
        }
        __syncthreads();
    }

    // ---- B: patch distances and weights ------------------------------------------------------------
    for (int item = tid; item < kNlmPix * T; item += kNlmThreads) {
        const int q = item & (kNlmPix - 1), t = item / kNlmPix;
        const int qy = q % kNlmTile, qx = q / kNlmTile;
        const int64_t gy = y0 + qy, gx = x0 + qx, cy = gy + t / nt - rs, cx = gx + t % nt - rs;
        float w = 0.0f;
        if (gy < a.H && gx < a.W && cy >= 0 && cy < a.H && cx >= 0 && cx < a.W) {
            double D = 0.0;
            for (int dx = 0; dx <= 2 * rp; ++dx)
                for (int dy = 0; dy <= 2 * rp; ++dy) D += (double)dacc[((qy + dy) + PH * (qx + dx)) * T + t];
            const double m = D / a.n - a.s2;
            w = (float)exp(-(m > 0.0 ? m * a.ih2 : 0.0));   // D = 0 (t = 0 among them): 1 exactly, whatever ih2
        }
        wts[q * T + t] = w;
    }
    __syncthreads();

    // ---- C: weighted sums --------------------------------------------------------------------------
    const int q = tid & (kNlmPix - 1), bl = tid / kNlmPix;
    const int kq = (q % kNlmTile + rp + rs) + E * (q / kNlmTile + rp + rs);
    const float *wq = wts + q * T;
    double den = 0.0;
    for (int t = 0; t < T; ++t) den += (double)wq[t];
    const int lv = a.lcb - NlmVec<V>::log2;
    for (int c0 = 0; c0 < a.B; c0 += a.cb) {
        const int cb = min(a.cb, a.B - c0);
        nlm_load<V>(a, pix, zs, E, S, rp, kNlmTile + 2 * rs, c0, cb);
        __syncthreads();
        double acc[kNlmMaxChunk / kNlmBandLanes];
#pragma unroll
        for (int j = 0; j < kNlmMaxChunk / kNlmBandLanes; ++j) acc[j] = 0.0;
        for (int tyi = 0; tyi < nt; ++tyi)
            for (int txi = 0; txi < nt; ++txi) {
                const double w = (double)wq[tyi * nt + txi];
                const float *zc = zs + (kq + (tyi - rs) + E * (txi - rs)) * S;
#pragma unroll
                for (int j = 0; j < kNlmMaxChunk / kNlmBandLanes; ++j) {
                    const int c = bl + kNlmBandLanes * j;
                    if (c < cb) acc[j] = fma(w, (double)zc[c], acc[j]);   // (the product is exact in fp64)
                }
            }
#pragma unroll
        for (int j = 0; j < kNlmMaxChunk / kNlmBandLanes; ++j) {
            const int c = bl + kNlmBandLanes * j;
            if (c < cb) outs[q * S + c] = (float)(acc[j] / den);
        }
        __syncthreads();
        for (int it = tid; it < (kNlmPix << lv); it += kNlmThreads) {
            const int c = (it & ((1 << lv) - 1)) * V, r = it >> lv;
            if (c >= cb || y0 + r % kNlmTile >= a.H || x0 + r / kNlmTile >= a.W) continue;
            const int k = (r % kNlmTile + rp + rs) + E * (r / kNlmTile + rp + rs);
            typename NlmVec<V>::type o;
            float *os = reinterpret_cast<float *>(&o);
#pragma unroll
            for (int j = 0; j < V; ++j) os[j] = outs[r * S + c + j];
            *reinterpret_cast<typename NlmVec<V>::type *>(a.U + (int64_t)pix[k] * a.B + c0 + c) = o;
        }
        // (the next chunk's load writes zs, which every thread has finished reading at the barrier above, and
        // outs is written again only after the next barrier)
    }
}

// H W B when every size is positive and the product is below 2^31, else 0 (bad sizes) or -1 (too large)
int64_t nlm_count(int64_t H, int64_t W, int64_t B) {
    if (H <= 0 || W <= 0 || B <= 0) return 0;
    const int64_t lim = (int64_t)1 << 31;
    if (H >= lim || W >= lim || B >= lim || H * W >= lim || H * W * B >= lim) return -1;
    return H * W * B;
}

size_t nlm_lds_bytes(int rp, int rs, int cb) {
    const size_t T = (size_t)(2 * rs + 1) * (2 * rs + 1), PH = kNlmTile + 2 * rp, E = PH + 2 * rs, S = cb + 1;
    return 4 * (PH * PH * T + kNlmPix * T + kNlmPix * S + E * E * S + E * E);
}

// Bands per chunk, a function of (rp, rs) alone: 32 when two workgroups then fit a CU's LDS, else the most
// that one workgroup can hold ((7, 5): 8 bands, 148 KiB)
int nlm_chunk(int rp, int rs) {
    if (nlm_lds_bytes(rp, rs, 32) <= kNlmLds / 2) return 32;
    return nlm_lds_bytes(rp, rs, 16) <= kNlmLds ? 16 : 8;
}

template <int V>
int nlm_run(const NlmArgs &a, size_t lds, unsigned grid, hipStream_t st) {
    static std::atomic<uint64_t> opted{0};   // dynamic LDS beyond 64 KiB, per device
    if (const int rc = lds_opt_in((const void *)k_nlmcube<V>, (int)kNlmLds, opted)) return rc;
    hipLaunchKernelGGL(k_nlmcube<V>, dim3(grid), dim3(kNlmThreads), lds, st, a);
    LRS_CHECK_LAUNCH();
    return LRS_OK;
}

inline bool nlm_aligned(const void *p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

}  // namespace

extern "C" size_t lrs_nlmcube_workspace(int64_t H, int64_t W, int64_t B, int patch_size, int patch_distance) {
    (void)H, (void)W, (void)B, (void)patch_size, (void)patch_distance;
    return 0;   // one launch; everything between its passes is in LDS
}

extern "C" int lrs_nlmcube_f32(const float *X, const float *L2, float c2, int64_t H, int64_t W, int64_t B,
                               int patch_size, int patch_distance, double h, double sigma, float *U, void *ws,
                               size_t ws_bytes, void *stream) {
    const size_t need = lrs_nlmcube_workspace(H, W, B, patch_size, patch_distance);
    if (!X || !U || (!ws && need > 0) || H <= 0 || W <= 0 || B <= 0 || patch_size < 1 || patch_size % 2 == 0 ||
        patch_distance < 0 || !(h > 0.0) || !isfinite(h) || !(sigma >= 0.0))
        return LRS_E_INVALID;
    const int64_t n = nlm_count(H, W, B);
    if (patch_size > 2 * kNlmMaxRp + 1 || patch_distance > kNlmMaxRs || n < 0) return LRS_E_UNSUPPORTED;
    if (ws_bytes < need) return LRS_E_WORKSPACE;
    const int rp = patch_size / 2, rs = patch_distance;
    NlmArgs a{X, L2, c2, U, (int)H, (int)W, (int)B, rp, rs, 0, 0, 0, 0.0, 0.0, 0.0};
    a.cb = nlm_chunk(rp, rs);
    a.lcb = a.cb == 32 ? 5 : a.cb == 16 ? 4 : 3;
    a.tiles_y = (int)((H + kNlmTile - 1) / kNlmTile);
    a.ih2 = (double)(float)(1.0 / (h * h));
    a.s2 = (double)(float)(2.0 * sigma * sigma);
    a.n = (double)B * (double)(patch_size * patch_size);
    const size_t lds = nlm_lds_bytes(rp, rs, a.cb);
    const unsigned grid = (unsigned)((int64_t)a.tiles_y * ((W + kNlmTile - 1) / kNlmTile));   // < 2^31 tiles: H W is
    hipStream_t st = (hipStream_t)stream;
    const bool al16 = nlm_aligned(X, 16) && nlm_aligned(L2, 16) && nlm_aligned(U, 16);
    const bool al8 = nlm_aligned(X, 8) && nlm_aligned(L2, 8) && nlm_aligned(U, 8);
    if (B % 4 == 0 && al16) return nlm_run<4>(a, lds, grid, st);
    if (B % 2 == 0 && al8) return nlm_run<2>(a, lds, grid, st);
    return nlm_run<1>(a, lds, grid, st);
}

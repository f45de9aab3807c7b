// DIP engine kernels outside the network: the unfolded-matrix <-> image transforms (plain and inside a
// reflected frame) and the parameter initialisation.  Part of dipnet.hip's translation unit: the
// kernels keep their internal linkage.
#pragma once

#include <stdint.h>

namespace {

__host__ __device__ inline uint64_t mix64(uint64_t z) {   // splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

__global__ void k_init_uniform(float *p, int64_t n, float bound, uint64_t key) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t z = mix64(key + 0x9e3779b97f4a7c15ULL * (uint64_t)(i + 1));
        const float u = (float)(z >> 40) * (1.0f / 16777216.0f);   // [0, 1)
        p[i] = (2.0f * u - 1.0f) * bound;
    }
}

__global__ void k_fill(float *p, int64_t n, float v) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        p[i] = v;
}

// img[b][i][j] = X[(i + H j) B + b] + c * L[...]   (…1-LiP.py:404; L nullable)
__global__ void k_unfolded_to_image(const float *__restrict__ X, const float *__restrict__ L, float c, int64_t H,
                                    int64_t W, int64_t B, float *__restrict__ img) {
    const int64_t n = H * W * B;
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < n; o += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = o % W, i = (o / W) % H, b = o / (W * H);
        const int64_t src = (i + H * j) * B + b;
        float v = X[src];
        if (L) v = v + c * L[src];
        img[o] = v;
    }
}

// X[(i + H j) B + b] = img[b][i][j]   (…1-LiP.py:411)
__global__ void k_image_to_unfolded(const float *__restrict__ img, int64_t H, int64_t W, int64_t B,
                                    float *__restrict__ X) {
    const int64_t n = H * W * B;
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < n; o += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = o % B, p = o / B;
        const int64_t i = p % H, j = p / H;
        X[o] = img[(b * H + i) * W + j];
    }
}

// ---- the same two transforms for an image inside a reflected frame (lrs_dipnet_set_frame) --------
// The image's H x W pixels sit at (top, left) of a Hf x Wf frame.  For one image row i both kernels
// transpose a 32 (columns j) x 32 (bands b) tile through LDS, so the unfolded rows X[(i + H j) B + b]
// are read / written along b and the image rows along j.
constexpr int kFrTile = 32;

struct FrameGeom {
    int H, W, B, top, left, Hf, Wf;
};

// The destinations of source index s along one axis of n pixels padded by lo before / hi after
// (ReflectionPad2d: the edge is not repeated): itself at lo + s, its mirror image in the leading pad
// (1 <= s <= lo) and in the trailing pad (n - 1 - hi <= s <= n - 2).  lo, hi < n.
__device__ __forceinline__ int frame_dests(int s, int n, int lo, int hi, int d[3]) {
    int nd = 0;
    d[nd++] = lo + s;
    if (s >= 1 && s <= lo) d[nd++] = lo - s;
    if (s >= n - 1 - hi && s <= n - 2) d[nd++] = 2 * (n - 1) + lo - s;
    return nd;
}

// img[b][top + i][left + j] = X[(i + H j) B + b] + c * L[...], and every frame pixel that reflects onto
// (i, j) in the same pass: the whole [B][Hf][Wf] image is written once, the unfolded rows are read once.
// grid (ceil(W / 32), ceil(B / 32), H), block (32, 8)
__global__ __launch_bounds__(256) void k_unfolded_to_frame(const float *__restrict__ X, const float *__restrict__ L,
                                                           float c, FrameGeom g, float *__restrict__ img) {
    __shared__ float tile[kFrTile][kFrTile + 1];   // [j][b]
    const int i = blockIdx.z, j0 = blockIdx.x * kFrTile, b0 = blockIdx.y * kFrTile;
    for (int r = threadIdx.y; r < kFrTile; r += blockDim.y) {   // lanes along b
        const int j = j0 + r, b = b0 + threadIdx.x;
        if (j < g.W && b < g.B) {
            const int64_t src = ((int64_t)i + (int64_t)g.H * j) * g.B + b;
            float v = X[src];
            if (L) v = v + c * L[src];
            tile[r][threadIdx.x] = v;
        }
    }
    __syncthreads();
    int ys[3];
    const int ny = frame_dests(i, g.H, g.top, g.Hf - g.H - g.top, ys);
    const int j = j0 + threadIdx.x;
    if (j >= g.W) return;
    int xs[3];
    const int nx = frame_dests(j, g.W, g.left, g.Wf - g.W - g.left, xs);
    for (int r = threadIdx.y; r < kFrTile; r += blockDim.y) {   // lanes along j
        const int b = b0 + r;
        if (b >= g.B) break;
        const float v = tile[threadIdx.x][r];
        float *plane = img + (int64_t)b * g.Hf * g.Wf;
        for (int a = 0; a < ny; ++a)
            for (int e = 0; e < nx; ++e) plane[(int64_t)ys[a] * g.Wf + xs[e]] = v;
    }
}

// X[(i + H j) B + b] = img[b][top + i][left + j]: the interior of the framed image, unfolded
__global__ __launch_bounds__(256) void k_frame_to_unfolded(const float *__restrict__ img, FrameGeom g,
                                                           float *__restrict__ X) {
    __shared__ float tile[kFrTile][kFrTile + 1];   // [b][j]
    const int i = blockIdx.z, j0 = blockIdx.x * kFrTile, b0 = blockIdx.y * kFrTile;
    for (int r = threadIdx.y; r < kFrTile; r += blockDim.y) {   // lanes along j
        const int b = b0 + r, j = j0 + threadIdx.x;
        if (b < g.B && j < g.W) tile[r][threadIdx.x] = img[((int64_t)b * g.Hf + g.top + i) * g.Wf + g.left + j];
    }
    __syncthreads();
    for (int r = threadIdx.y; r < kFrTile; r += blockDim.y) {   // lanes along b
        const int j = j0 + r, b = b0 + threadIdx.x;
        if (j < g.W && b < g.B) X[((int64_t)i + (int64_t)g.H * j) * g.B + b] = tile[threadIdx.x][r];
    }
}

}  // namespace

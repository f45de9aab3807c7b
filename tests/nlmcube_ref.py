"""The spectral non-local-means prox on the cube (lrs_nlmcube_f32, include/lrspnp.h) restated for tests, in
fp64 numpy.

The cube is z[c][y][x], shape (B, H, W); `image` / `unfolded` convert from and to the library's [P][B] layout
(p = y + H x).  With rp = patch_size // 2, rs = patch_distance, ih2 = float32(1 / h^2), s2 = float32(2 sigma^2):
    m(e) on an axis of length n: 0 when n = 1, else r = e mod 2 (n - 1), r when r < n and 2 (n - 1) - r otherwise
    d(e, e') = sum_c (z[c, m(e)] - z[c, m(e')])^2
    D(p, t)  = sum_{|dy|, |dx| <= rp} d(p + delta, p + delta + t)
    w(p, t)  = exp(-max(D(p, t) / (B (2 rp + 1)^2) - s2, 0) ih2)
    U[c, p]  = sum_t w(p, t) z[c, p + t] / sum_t w(p, t)
over the offsets |ty|, |tx| <= rs whose candidate p + t lies inside the image.  Everything but ih2 and s2 is fp64.
"""
from __future__ import annotations

import numpy as np


def image(X, H, W):
    """(P, B) unfolded -> (B, H, W)."""
    X = np.asarray(X)
    return np.ascontiguousarray(X.reshape(W, H, X.shape[1]).transpose(2, 1, 0))


def unfolded(o):
    """(B, H, W) -> (P, B)."""
    B, H, W = o.shape
    return np.ascontiguousarray(np.asarray(o).transpose(2, 1, 0).reshape(H * W, B))


def reflect(e, n):
    """m(e): reflection without repeating the edge, continued periodically."""
    e = np.asarray(e)
    if n == 1:
        return np.zeros_like(e)
    per = 2 * (n - 1)
    r = np.mod(e, per)
    return np.where(r < n, r, per - r)


def params(h, sigma):
    """(ih2, s2) as the library's host rounds them, once, to float32."""
    return float(np.float32(1.0 / (float(h) * float(h)))), float(np.float32(2.0 * float(sigma) * float(sigma)))


def offsets(patch_distance):
    rs = int(patch_distance)
    return [(ty, tx) for ty in range(-rs, rs + 1) for tx in range(-rs, rs + 1)]


def patch_distances(z, patch_size, patch_distance):
    """{(ty, tx): D(., t) of shape (H, W)} for every offset of the window, whether or not the candidate is inside."""
    z = np.asarray(z, np.float64)
    B, H, W = z.shape
    rp, rs = int(patch_size) // 2, int(patch_distance)
    pad = rp + rs
    e = z[:, reflect(np.arange(-pad, H + pad), H)][:, :, reflect(np.arange(-pad, W + pad), W)]
    a = e[:, rs:rs + H + 2 * rp, rs:rs + W + 2 * rp]
    out = {}
    for ty, tx in offsets(rs):
        b = e[:, rs + ty:rs + ty + H + 2 * rp, rs + tx:rs + tx + W + 2 * rp]
        d = ((a - b) ** 2).sum(0)
        D = np.zeros((H, W))
        for dy in range(2 * rp + 1):
            for dx in range(2 * rp + 1):
                D += d[dy:dy + H, dx:dx + W]
        out[(ty, tx)] = D
    return out


def inside(H, W, ty, tx):
    """(H, W) bool: the candidate p + t lies inside the image."""
    ys, xs = np.arange(H)[:, None] + ty, np.arange(W)[None, :] + tx
    return (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)


def nlm(z, patch_size=7, patch_distance=2, h=0.05, sigma=0.0):
    """U (B, H, W) fp64 of the cube z (B, H, W)."""
    z = np.asarray(z, np.float64)
    B, H, W = z.shape
    ih2, s2 = params(h, sigma)
    n = B * (2 * (int(patch_size) // 2) + 1) ** 2
    num, den = np.zeros_like(z), np.zeros((H, W))
    for (ty, tx), D in patch_distances(z, patch_size, patch_distance).items():
        ok = inside(H, W, ty, tx)
        w = np.where(ok, np.exp(-np.maximum(D / n - s2, 0.0) * ih2), 0.0)
        ys = np.clip(np.arange(H)[:, None] + ty, 0, H - 1)
        xs = np.clip(np.arange(W)[None, :] + tx, 0, W - 1)
        num += w * z[:, ys, xs]
        den += w
    return num / den


def window_mean(z, patch_distance):
    """The mean over the clipped search window: what nlm() returns when every weight is 1."""
    z = np.asarray(z, np.float64)
    B, H, W = z.shape
    num, den = np.zeros_like(z), np.zeros((H, W))
    for ty, tx in offsets(patch_distance):
        ok = inside(H, W, ty, tx)
        ys = np.clip(np.arange(H)[:, None] + ty, 0, H - 1)
        xs = np.clip(np.arange(W)[None, :] + tx, 0, W - 1)
        num += ok * z[:, ys, xs]
        den += ok
    return num / den


def denoising_case(seed=0):
    """(clean, noisy) (8, 24, 20): a piecewise-constant cube of 4 materials and N(0, 0.05^2) noise."""
    rng = np.random.default_rng(seed)
    B, H, W = 8, 24, 20
    lab = (np.arange(H)[:, None] // 8 + 2 * (np.arange(W)[None, :] // 7)) % 4
    clean = rng.random((4, B))[lab].transpose(2, 0, 1)
    return clean, clean + 0.05 * rng.standard_normal(clean.shape)

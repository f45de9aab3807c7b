"""The TV prox on the cube (lrs_tvprox_f32, include/lrspnp.h) restated for tests, in fp64 numpy.

The cube is o[c][y][x], shape (B, H, W); `image` / `unfolded` convert from and to the library's [P][B] layout
(p = i + H j, o[b][i][j] = X[p][b]).  K stacks the difference fields of the terms whose weight is > 0, out of
    y: o[c,y+1,x] - o[c,y,x]     x: o[c,y,x+1] - o[c,y,x]     c: o[c+1,y,x] - o[c,y,x]
    yc: (o[c+1,y+1,x] - o[c,y+1,x]) - (o[c+1,y,x] - o[c,y,x])     xc: likewise along x,
each over the indices whose operands all lie inside the cube (an empty array for a dimension of 1).
    U = argmin_u 1/2 ||u - z||^2 + tau T(u),  T(u) = w_sp (|y| + |x|) + w_bd |c| + w_ss (|yc| + |xc|) summed,
by the fast gradient projection on the dual, step for step as the library runs it: radii r = float32(tau w),
step float32(1 / L) with L = 8 [w_sp > 0] + 4 [w_bd > 0] + 32 [w_ss > 0], t in fp64 and beta rounded once to
float32; everything else in fp64.
"""
from __future__ import annotations

import numpy as np

FIELDS = ("y", "x", "c", "yc", "xc")


def weights(w_sp=0.0, w_bd=0.0, w_ss=0.0):
    """{field: weight} of the active fields (weight > 0), in K's order."""
    w = {"y": w_sp, "x": w_sp, "c": w_bd, "yc": w_ss, "xc": w_ss}
    return {f: float(w[f]) for f in FIELDS if w[f] > 0}


def lipschitz(w_sp=0.0, w_bd=0.0, w_ss=0.0):
    return 8.0 * (w_sp > 0) + 4.0 * (w_bd > 0) + 32.0 * (w_ss > 0)


def image(X, H, W):
    """(P, B) unfolded -> (B, H, W)."""
    X = np.asarray(X)
    return np.ascontiguousarray(X.reshape(W, H, X.shape[1]).transpose(2, 1, 0))


def unfolded(o):
    """(B, H, W) -> (P, B)."""
    B, H, W = o.shape
    return np.ascontiguousarray(np.asarray(o).transpose(2, 1, 0).reshape(H * W, B))


def K(u, fields):
    """{field: its differences of u}."""
    e = u[1:] - u[:-1]
    d = {"y": lambda: u[:, 1:, :] - u[:, :-1, :], "x": lambda: u[:, :, 1:] - u[:, :, :-1], "c": lambda: e,
         "yc": lambda: e[:, 1:, :] - e[:, :-1, :], "xc": lambda: e[:, :, 1:] - e[:, :, :-1]}
    return {f: d[f]() for f in fields}


def Kt(p, shape):
    """K^T p for p = {field: array}, an array of `shape`."""
    B = shape[0]
    g = np.zeros(shape)
    ge = np.zeros((max(B - 1, 0),) + tuple(shape[1:]))   # the adjoint with respect to the band difference
    for f, v in p.items():
        t = ge if f in ("yc", "xc") else g
        if f in ("y", "yc"):
            t[:, 1:, :] += v
            t[:, :-1, :] -= v
        elif f in ("x", "xc"):
            t[:, :, 1:] += v
            t[:, :, :-1] -= v
        else:
            g[1:] += v
            g[:-1] -= v
    g[1:] += ge
    g[:-1] -= ge
    return g


def regulariser(u, w_sp=0.0, w_bd=0.0, w_ss=0.0):
    """T(u)."""
    w = weights(w_sp, w_bd, w_ss)
    return float(sum(w[f] * np.abs(v).sum() for f, v in K(np.asarray(u, np.float64), w).items()))


def radii(w_sp, w_bd, w_ss, tau):
    """{field: the fp32 box radius the iteration clips to}."""
    return {f: float(np.float32(tau * w)) for f, w in weights(w_sp, w_bd, w_ss).items()}


def objective(U, z, w_sp=0.0, w_bd=0.0, w_ss=0.0, tau=0.0):
    """1/2 ||U - z||^2 + tau T(U)."""
    U, z = np.asarray(U, np.float64), np.asarray(z, np.float64)
    return 0.5 * float(((U - z) ** 2).sum()) + tau * regulariser(U, w_sp, w_bd, w_ss)


def gap(U, p, w_sp=0.0, w_bd=0.0, w_ss=0.0, tau=0.0):
    """sum_f r_f |K_f U| - <p, K U> with the fp32 radii (every term is >= 0 for |p| <= r)."""
    r = radii(w_sp, w_bd, w_ss, tau)
    d = K(np.asarray(U, np.float64), r)
    return float(sum((r[f] * np.abs(d[f]) - p[f] * d[f]).sum() for f in r))


def betas(n_iter):
    """beta_1 .. beta_n: t in fp64, beta rounded once to float32 (LRS_ISTA_ACCEL_FISTA's convention)."""
    t, out = 1.0, []
    for _ in range(n_iter):
        tn = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
        out.append(float(np.float32((t - 1.0) / tn)))
        t = tn
    return out


def fgp(z, w_sp=0.0, w_bd=0.0, w_ss=0.0, tau=0.0, n_iter=0, p0=None):
    """(U, p) after n_iter iterations from p0 (None: 0; else clipped to the radii), z of shape (B, H, W)."""
    z = np.asarray(z, np.float64)
    r = radii(w_sp, w_bd, w_ss, tau)
    if not r or tau == 0 or n_iter == 0:
        return z.copy(), {f: np.zeros_like(v) for f, v in K(z, r).items()}
    inv_l = float(np.float32(1.0) / np.float32(lipschitz(w_sp, w_bd, w_ss)))
    if p0 is None:
        p = {f: np.zeros_like(v) for f, v in K(z, r).items()}
    else:
        p = {f: np.clip(p0[f], -r[f], r[f]) for f in r}
    q = {f: v.copy() for f, v in p.items()}
    for beta in betas(n_iter):
        d = K(z - Kt(q, z.shape), r)
        pn = {f: np.clip(q[f] + inv_l * d[f], -r[f], r[f]) for f in r}
        q = {f: pn[f] + beta * (pn[f] - p[f]) for f in r}
        p = pn
    return z - Kt(p, z.shape), p

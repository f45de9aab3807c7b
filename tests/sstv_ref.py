"""The DIP loss's smoothness term (lrs_sstv_f32, include/lrspnp.h) restated for tests, in fp64.

With N = n_mean (default C*H*W) and phi(d) = sqrt(d^2 + eps^2) (|d| for eps = 0), for an image o[C][H][W]:
    R(o) = (w_sp / N) sum [ phi(o[c,y+1,x] - o[c,y,x]) + phi(o[c,y,x+1] - o[c,y,x]) ]
         + (w_bd / N) sum   phi(o[c+1,y,x] - o[c,y,x])
         + (w_ss / N) sum [ phi(Dy Dc o) + phi(Dx Dc o) ]
    Dy Dc o[c,y,x] = (o[c+1,y+1,x] - o[c,y+1,x]) - (o[c+1,y,x] - o[c,y,x]),  Dx Dc likewise along x,
every sum over the indices whose operands all lie inside the image (no padding).

closed_form: numpy, R and dR/do written out term by term (phi'(d) = d / sqrt(d^2 + eps^2); eps = 0: sign(d) with
sign(0) = 0).  term: the same R from torch ops in the input's dtype, for autograd (torch's abs backward is sign).
grid_image: inputs on the grid of multiples of 2^-6 in [0, 4), on which every first and second difference is
exact in fp32 and fp64, with exact ties planted; zero_counts: how many differences of each kind are zero.
"""
from __future__ import annotations

import numpy as np
import torch


def _phi(d, eps):
    return np.sqrt(d * d + eps * eps) if eps > 0 else np.abs(d)


def _dphi(d, eps):
    return d / np.sqrt(d * d + eps * eps) if eps > 0 else np.sign(d)


def closed_form(o, w_sp=0.0, w_bd=0.0, w_ss=0.0, eps=0.0, n_mean=None):
    """(R, dR/do) of the (C, H, W) image o, fp64 numpy."""
    o = np.asarray(o, np.float64)
    assert o.ndim == 3
    N = float(o.size if n_mean is None else n_mean)
    g = np.zeros_like(o)
    R = 0.0
    # spatial: along y, then along x
    d = o[:, 1:, :] - o[:, :-1, :]
    R += w_sp * _phi(d, eps).sum()
    p = w_sp * _dphi(d, eps)
    g[:, 1:, :] += p
    g[:, :-1, :] -= p
    d = o[:, :, 1:] - o[:, :, :-1]
    R += w_sp * _phi(d, eps).sum()
    p = w_sp * _dphi(d, eps)
    g[:, :, 1:] += p
    g[:, :, :-1] -= p
    # band
    e = o[1:] - o[:-1]
    R += w_bd * _phi(e, eps).sum()
    p = w_bd * _dphi(e, eps)
    g[1:] += p
    g[:-1] -= p
    # spatial-spectral: the spatial differences of the band difference e
    ge = np.zeros_like(e)
    q = e[:, 1:, :] - e[:, :-1, :]
    R += w_ss * _phi(q, eps).sum()
    p = w_ss * _dphi(q, eps)
    ge[:, 1:, :] += p
    ge[:, :-1, :] -= p
    q = e[:, :, 1:] - e[:, :, :-1]
    R += w_ss * _phi(q, eps).sum()
    p = w_ss * _dphi(q, eps)
    ge[:, :, 1:] += p
    ge[:, :, :-1] -= p
    g[1:] += ge
    g[:-1] -= ge
    return R / N, g / N


def term(o, w_sp=0.0, w_bd=0.0, w_ss=0.0, eps=0.0, n_mean=None):
    """R of the (C, H, W) tensor o as a torch scalar in o's dtype (differentiable)."""
    def phi(d):
        return torch.sqrt(d * d + eps * eps) if eps > 0 else d.abs()
    N = float(o.numel() if n_mean is None else n_mean)
    e = o[1:] - o[:-1]
    R = w_sp * (phi(o[:, 1:, :] - o[:, :-1, :]).sum() + phi(o[:, :, 1:] - o[:, :, :-1]).sum())
    R = R + w_bd * phi(e).sum()
    R = R + w_ss * (phi(e[:, 1:, :] - e[:, :-1, :]).sum() + phi(e[:, :, 1:] - e[:, :, :-1]).sum())
    return R / N


def autograd(o, w_sp=0.0, w_bd=0.0, w_ss=0.0, eps=0.0, n_mean=None):
    """(R, dR/do) by torch autograd in fp64, as numpy."""
    t = torch.as_tensor(np.asarray(o, np.float64)).clone().requires_grad_(True)
    R = term(t, w_sp, w_bd, w_ss, eps, n_mean)
    if not R.requires_grad:     # every sum empty (a 1 x 1 x 1 image)
        return float(R), np.zeros(t.shape)
    R.backward()
    return float(R.detach()), t.grad.numpy()


def grid_image(shape, seed=0):
    """(C, H, W) float32 on the grid k / 64, k in [0, 256), with exact ties planted in the corner at the
    origin wherever the shape has room: equal neighbours along y, x and c, and a 2 x 2 (band, row) and
    (band, column) block of equal values, so that a zero first difference of each direction and a zero
    second difference of each kind occur."""
    C, H, W = shape
    rng = np.random.default_rng(1000 + seed + 101 * C + 10007 * H + 1000003 * W)
    o = rng.integers(0, 256, size=shape).astype(np.float32) / 64.0
    a = o[0, 0, 0]
    if H > 1:
        o[0, 1, 0] = a
    if W > 1:
        o[0, 0, 1] = a
    if C > 1:
        o[1, 0, 0] = a
        if H > 1:
            o[1, 1, 0] = a
        if W > 1:
            o[1, 0, 1] = a
    return o


def zero_counts(o):
    """{kind: the number of exactly zero differences of that kind} for kinds dy, dx, dc, qy, qx."""
    o = np.asarray(o, np.float64)
    e = o[1:] - o[:-1]
    d = {"dy": o[:, 1:, :] - o[:, :-1, :], "dx": o[:, :, 1:] - o[:, :, :-1], "dc": e,
         "qy": e[:, 1:, :] - e[:, :-1, :], "qx": e[:, :, 1:] - e[:, :, :-1]}
    return {k: int((v == 0).sum()) for k, v in d.items()}


def kinds_possible(shape):
    """The kinds of difference an image of this shape has at all."""
    C, H, W = shape
    return {"dy": H > 1, "dx": W > 1, "dc": C > 1, "qy": C > 1 and H > 1, "qx": C > 1 and W > 1}

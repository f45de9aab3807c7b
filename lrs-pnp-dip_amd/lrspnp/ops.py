"""Tensor-level wrappers over the C ABI (include/lrspnp.h).

torch is only plumbing here: device memory, the current HIP stream, dtype/shape checks.  Every
arithmetic step runs in liblrspnp_hip.so; nothing falls back to torch/numpy compute.
"""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np
import torch

from ._lib import (ALPHA_FRO4, ALPHA_SOFT, ALPHA_SPEC2, ISTA_SPLIT_BF16, PROX_NLM, PROX_NLM_MATLAB, PROX_SOFT,
                   SVT_JACOBI, SVT_MULTI_WG, SVT_WARM, SVT_WIDE_MW, SVT_WIDE_TRI, TVPROX_WARM, LrsError, check, dev,
                   device_lib, ista_accel, ista_opts, lib, mask_channels, outs, ptr, sptr)

__all__ = ["nlm_col", "block_grid", "cover_ranges", "im2col", "ista_alpha", "ista", "svt_workspace", "svt_max_bands",
           "ista_workspace", "ista_pat_plan", "ista_pat_preferred", "ista_pat_workspace", "ista_pat_prepare",
           "ista_pat", "dict_workspace", "dict_stats", "dict_update", "dict_normalise", "nlm_matlab_col", "svt",
           "svt_gram", "svt_gram_view", "svt_finish", "svt_plan", "svt_state", "svt_apply_only", "SVT_CHAINS",
           "tvprox_workspace", "tvprox", "nlmcube_workspace", "nlmcube", "cube_quality_workspace", "cube_quality",
           "keep_best", "admm_update", "unfolded_to_image", "image_to_unfolded", "unfolded_to_frame",
           "frame_to_unfolded", "masked_mse", "sstv", "mask_channels", "ALPHA_SPEC2", "ALPHA_FRO4", "ALPHA_SOFT",
           "PROX_NLM", "PROX_SOFT", "PROX_NLM_MATLAB"]


# ---------------------------------------------------------------------------------------------
def _nlm_rows(entry: str, g, h, out, stream, *patch):
    """The NLM entry point `entry` (lrs_nlm_col_f32 with its patch sizes, lrs_nlm_matlab_col_f32 without) on
    every row of g (nvec, K) or on the one vector g (K,); h: float or a float64 device tensor (nvec,)."""
    L = device_lib()
    g = dev(g, torch.float32, "g")
    g2 = g.view(1, -1) if g.dim() == 1 else g
    nvec, K = g2.shape
    o = torch.empty_like(g2) if out is None else dev(out, torch.float32, "out").view(nvec, K)
    hv, hs = (dev(h, torch.float64, "h"), 0.0) if isinstance(h, torch.Tensor) else (None, float(h))
    check(getattr(L, entry)(ptr(g2), K, ptr(o), K, K, nvec, hs, ptr(hv), *patch, sptr(stream)), entry)
    return o.view_as(g)


def nlm_col(g: torch.Tensor, h, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """NLM prox of every row of g (nvec, K): skimage denoise_nl_means(g_v[:,None], h, fast_mode=True,
    patch_size=3, patch_distance=3) per vector.  h: float or a float64 device tensor (nvec,)."""
    return _nlm_rows("lrs_nlm_col_f32", g, h, out, stream, 3, 3)


def block_grid(P: int, B: int, bb: int, sliding: int):
    """get_image_block corners (host int32 arrays), in the reference's order."""
    L = lib()
    nb = L.lrs_block_count(P, B, bb, sliding)
    if nb < 0:
        check(int(nb), "lrs_block_count")
    rows = np.empty(nb, np.int32)
    cols = np.empty(nb, np.int32)
    i32p = ctypes.POINTER(ctypes.c_int32)
    check(L.lrs_block_grid(P, B, bb, sliding, rows.ctypes.data_as(i32p), cols.ctypes.data_as(i32p), nb),
          "lrs_block_grid")
    return rows, cols


def cover_ranges(extent: int, bb: int, starts: np.ndarray):
    L = lib()
    starts = np.ascontiguousarray(starts, np.int32)
    lo = np.empty(extent, np.int32)
    hi = np.empty(extent, np.int32)
    i32p = ctypes.POINTER(ctypes.c_int32)
    check(L.lrs_cover_ranges(extent, bb, starts.ctypes.data_as(i32p), starts.size, lo.ctypes.data_as(i32p),
                             hi.ctypes.data_as(i32p)), "lrs_cover_ranges")
    return lo, hi


def im2col(X, Lm, mu: float, bb: int, rows_d, cols_d, n_pad: int, Yb=None, obs=None, want_obs=False,
           stream=None):
    """Yb[j] = block j of (X + Lm/mu) flattened F-order (get_image_block), zero-padded to n_pad."""
    L = device_lib()
    X = dev(X, torch.float32, "X")
    if Lm is not None:
        dev(Lm, torch.float32, "L")
    P, B = X.shape
    nb = rows_d.numel()
    if Yb is None:
        Yb = torch.empty((nb, n_pad), dtype=torch.float32, device=X.device)
    if want_obs and obs is None:
        obs = torch.empty((nb, n_pad), dtype=torch.uint8, device=X.device)
    check(L.lrs_im2col_f32(ptr(X), ptr(Lm), float(mu), P, B, bb, ptr(rows_d), ptr(cols_d), nb, n_pad, ptr(Yb),
                           ptr(obs) if want_obs else None, sptr(stream)), "lrs_im2col_f32")
    return (Yb, obs) if want_obs else Yb


def ista_alpha(D, obs_pat, n: int, mode: int, lambda_ista: float, stream=None):
    L = device_lib()
    D = dev(D, torch.float32, "D")
    obs_pat = dev(obs_pat, torch.uint8, "obs_pat")
    nD, K = D.shape
    npat, n_pad = obs_pat.shape
    alpha = torch.empty(npat, dtype=torch.float32, device=D.device)
    thr = torch.empty(npat, dtype=torch.float64, device=D.device)
    wsb = L.lrs_ista_alpha_workspace(n, K, npat)
    ws = torch.empty(max(int(wsb), 1), dtype=torch.uint8, device=D.device)
    check(L.lrs_ista_alpha_f32(ptr(D), n, K, ptr(obs_pat), npat, n_pad, mode, float(lambda_ista), ptr(alpha),
                               ptr(thr), ptr(ws), ws.numel(), sptr(stream)), "lrs_ista_alpha_f32")
    return alpha, thr


def ista_workspace(n: int, K: int, prox: int, device, algorithm: int = 0, accel: str = "off") -> torch.Tensor | None:
    """Device workspace of lrs_ista_f32 (the row-split kernel's fragment-ordered dictionary images,
    or the generic path's chunk buffers for K > 512); None when the dictionary-resident kernels serve
    (n <= 64, K = 256, skimage / soft prox, accel "off").  Query it with the call's own algorithm and
    accel: "fista" runs the row-split kernel at the resident sizes too, and the generic path then
    keeps one more chunk of coefficients."""
    acc = ista_accel(accel)
    opts = ctypes.byref(ista_opts(algorithm=int(algorithm), accel=acc)) if algorithm or acc else None
    nbytes = int(lib().lrs_ista_workspace(int(n), int(K), int(prox), opts))
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


def _ista_prep(who: str, Yb, K: int, phi, coefs, want_coefs, warm_start, accel, max_workgroups, precision=None,
               algorithm: int = 0):
    """What ista() and ista_pat() prepare alike: phi and coefs allocated where absent, the warm-start rule, and
    this call's lrs_ista_opts (None = the library defaults).  Returns (phi, coefs or None when not wanted, opts)."""
    nb, n_pad = Yb.shape
    if phi is None:
        phi = torch.empty((nb, n_pad), dtype=torch.float32, device=Yb.device)
    if warm_start:
        if coefs is None:
            raise LrsError(f"{who}(warm_start=True) continues from `coefs`: pass it")
        want_coefs = True
    if want_coefs and coefs is None:
        coefs = torch.empty((nb, K), dtype=torch.float32, device=Yb.device)
    acc = ista_accel(accel)
    opts = None
    if precision is not None or max_workgroups or algorithm or warm_start or acc:
        opts = ctypes.byref(ista_opts(ISTA_SPLIT_BF16 if precision is None else int(precision), int(max_workgroups),
                                      int(algorithm), 1 if warm_start else 0, acc))
    return phi, coefs if want_coefs else None, opts


def ista(Yb, obs, D, n: int, alpha, thr, Nit: int, prox: int = PROX_NLM, phi=None, coefs=None,
         want_coefs=False, ws=None, stream=None, precision: int | None = None, max_workgroups: int = 0,
         algorithm: int = 0, warm_start: bool = False, accel: str = "off"):
    """Masked ISTA + prox over all blocks; returns phi (nb, n_pad) [, coefs (nb, K)].  `ws`: an
    ista_workspace() buffer (allocated here when None and needed).  precision / max_workgroups /
    algorithm / warm_start / accel: this call's lrs_ista_opts (None / 0 = the library defaults; algorithm 1 =
    the generic dense-GEMM path that K > 512 always takes; warm_start: continue from `coefs`, which
    must be given, and write the result back to it; accel "fista": Nesterov momentum on the same
    gradient step and prox (include/lrspnp.h), restarted by every call, so warm-started slices of an
    accelerated run are not one call)."""
    L = device_lib()
    dev(Yb, torch.float32, "Yb")
    dev(obs, torch.uint8, "obs")
    dev(D, torch.float32, "D")
    dev(alpha, torch.float32, "alpha")
    dev(thr, torch.float64, "thr")
    nb, n_pad = Yb.shape
    K = D.shape[1]
    phi, coefs, opts = _ista_prep("ista", Yb, K, phi, coefs, want_coefs, warm_start, accel, max_workgroups, precision,
                                  algorithm)
    if ws is None:
        ws = ista_workspace(n, K, prox, Yb.device, algorithm, accel)
    check(L.lrs_ista_f32(ptr(Yb), ptr(obs), ptr(D), n, n_pad, K, nb, ptr(alpha), ptr(thr), int(Nit), int(prox),
                         ptr(coefs), ptr(phi), opts, ptr(ws), 0 if ws is None else ws.numel(), sptr(stream)),
          "lrs_ista_f32")
    return phi if coefs is None else (phi, coefs)


def ista_pat_plan(pat, npat: int):
    """Blocks grouped by observation pattern (lrs_ista_pat_plan, host): returns (plan int32 numpy
    array, ntiles).  pat: block j's pattern index in [0, npat) (host int32 array)."""
    L = lib()
    pat = np.ascontiguousarray(np.asarray(pat), dtype=np.int32)
    nb = pat.size
    cap = int(L.lrs_ista_pat_plan_len(nb, int(npat)))
    if cap < 0:
        check(cap, "lrs_ista_pat_plan_len")
    plan = np.zeros(cap, np.int32)
    i32p = ctypes.POINTER(ctypes.c_int32)
    nt = int(L.lrs_ista_pat_plan(pat.ctypes.data_as(i32p), nb, int(npat), plan.ctypes.data_as(i32p), cap))
    if nt < 0:
        check(nt, "lrs_ista_pat_plan")
    return plan, nt


def ista_pat_preferred(n: int, K: int, nb: int, npat: int, Nit: int) -> bool:
    """Whether the per-pattern Gram path does less matrix-core work than the row-split kernel."""
    return bool(lib().lrs_ista_pat_preferred(int(n), int(K), int(nb), int(npat), int(Nit)))


def ista_pat_workspace(n: int, K: int, npat: int, device) -> torch.Tensor:
    return torch.empty(max(int(lib().lrs_ista_pat_workspace(int(n), int(K), int(npat))), 1), dtype=torch.uint8,
                       device=device)


def ista_pat_prepare(D, obs_pat, n: int, ws=None, stream=None) -> torch.Tensor:
    """The dictionary images and every pattern's masked Gram Q_p = D^T diag(m_p) D in `ws`
    (lrs_ista_pat_prepare; allocated here when None); returns ws, which ista_pat() then reads."""
    L = device_lib()
    dev(D, torch.float32, "D")
    dev(obs_pat, torch.uint8, "obs_pat")
    K = D.shape[1]
    npat, n_pad = obs_pat.shape
    if ws is None:
        ws = ista_pat_workspace(n, K, npat, D.device)
    check(L.lrs_ista_pat_prepare(ptr(D), n, K, ptr(obs_pat), npat, n_pad, ptr(ws), ws.numel(), sptr(stream)),
          "lrs_ista_pat_prepare")
    return ws


def ista_pat(Yb, obs_pat, plan, ntiles: int, K: int, n: int, alpha, thr, Nit: int, ws, prox: int = PROX_NLM,
             phi=None, coefs=None, want_coefs=False, stream=None, max_workgroups: int = 0, warm_start: bool = False,
             accel: str = "off"):
    """Masked ISTA + prox on per-pattern Grams (lrs_ista_pat_f32) for blocks that share observation
    patterns, on the images ista_pat_prepare() left in `ws`.  obs_pat (npat, n_pad) u8 and plan
    (ista_pat_plan's, as an int32 device tensor) on the device; the rest as ista(), accel included.
    Returns phi [, coefs]."""
    L = device_lib()
    dev(Yb, torch.float32, "Yb")
    dev(obs_pat, torch.uint8, "obs_pat")
    dev(plan, torch.int32, "plan")
    dev(alpha, torch.float32, "alpha")
    dev(thr, torch.float64, "thr")
    dev(ws, torch.uint8, "ws")
    nb, n_pad = Yb.shape
    npat = obs_pat.shape[0]
    phi, coefs, opts = _ista_prep("ista_pat", Yb, K, phi, coefs, want_coefs, warm_start, accel, max_workgroups)
    check(L.lrs_ista_pat_f32(ptr(Yb), ptr(obs_pat), npat, ptr(plan), int(ntiles), n, n_pad, int(K), nb, ptr(alpha),
                             ptr(thr), int(Nit), int(prox), ptr(coefs), ptr(phi), opts, ptr(ws), ws.numel(),
                             sptr(stream)), "lrs_ista_pat_f32")
    return phi if coefs is None else (phi, coefs)


def dict_workspace(n: int, n_pad: int, K: int, nb: int, device) -> torch.Tensor:
    """Device workspace of dict_stats() / dict_update() at these sizes (lrs_dict_workspace)."""
    nbytes = int(lib().lrs_dict_workspace(int(n), int(n_pad), int(K), int(nb)))
    if nbytes == 0:
        raise LrsError(f"lrs_dict_workspace: sizes not served (n {n}, n_pad {n_pad}, K {K}, nb {nb}; K <= 512)")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def dict_stats(coefs, H=None, c=None, ws=None, stream=None):
    """H = coefs^T coefs (K, K) float32 and c = max_k sum_l |H_kl| (a float64 device tensor of one
    element: Gershgorin's bound on lambda_max(H), the dictionary step's 1 / step size)."""
    L = device_lib()
    dev(coefs, torch.float32, "coefs")
    nb, K = coefs.shape
    if H is None:
        H = torch.empty((K, K), dtype=torch.float32, device=coefs.device)
    if c is None:
        c = torch.empty(1, dtype=torch.float64, device=coefs.device)
    dev(H, torch.float32, "H")
    dev(c, torch.float64, "c")
    if ws is None:
        ws = dict_workspace(16, 16, K, nb, coefs.device)
    check(L.lrs_dict_stats_f32(ptr(coefs), nb, K, ptr(H), ptr(c), ptr(ws), ws.numel(), sptr(stream)),
          "lrs_dict_stats_f32")
    return H, c


def dict_update(Yb, obs, coefs, D, n: int, c, n_inner: int, obj=None, ws=None, stream=None):
    """n_inner majorisation-minimisation iterations of the masked dictionary step, in place on D
    (n, K): u_k = d_k + (R^T coefs)_k / c, d_k = u_k / max(1, ||u_k||), R = obs .* (Yb - coefs D^T).
    c: dict_stats()'s device scalar.  Returns obj (n_inner + 1,) float64 on the device: 1/2 ||R||^2
    before each iteration and after the last."""
    L = device_lib()
    dev(Yb, torch.float32, "Yb")
    dev(obs, torch.uint8, "obs")
    dev(coefs, torch.float32, "coefs")
    dev(D, torch.float32, "D")
    dev(c, torch.float64, "c")
    nb, n_pad = Yb.shape
    K = D.shape[1]
    if D.shape[0] != n or coefs.shape != (nb, K) or obs.shape != Yb.shape:
        raise LrsError(f"dict_update: D {tuple(D.shape)}, coefs {tuple(coefs.shape)}, obs {tuple(obs.shape)} do not "
                       f"match Yb {tuple(Yb.shape)} with n = {n}")
    if obj is None:
        obj = torch.empty(int(n_inner) + 1, dtype=torch.float64, device=Yb.device)
    dev(obj, torch.float64, "obj")
    if obj.numel() < int(n_inner) + 1:
        raise LrsError("dict_update: obj holds fewer than n_inner + 1 values")
    if ws is None:
        ws = dict_workspace(n, n_pad, K, nb, Yb.device)
    check(L.lrs_dict_update_f32(ptr(Yb), ptr(obs), ptr(coefs), ptr(D), n, n_pad, K, nb, ptr(c), int(n_inner), ptr(obj),
                                ptr(ws), ws.numel(), sptr(stream)), "lrs_dict_update_f32")
    return obj


def dict_normalise(D, stream=None):
    """Every column of D (n, K) with a non-zero norm scaled to unit norm, in place (columnNormalise.m)."""
    L = device_lib()
    dev(D, torch.float32, "D")
    check(L.lrs_dict_normalise_f32(ptr(D), D.shape[0], D.shape[1], sptr(stream)), "lrs_dict_normalise_f32")
    return D


def nlm_matlab_col(g: torch.Tensor, h, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """NLmeansfilter(g_v, 3, 3, h) (LRS-PnP(Matlab Code)/NLmeansfilter.m) of every row of g (nvec, K)."""
    return _nlm_rows("lrs_nlm_matlab_col_f32", g, h, out, stream)


def svt_max_bands() -> int:
    """The largest band count the SVT calls accept (lrs_svt_max_bands; host-only)."""
    return int(lib().lrs_svt_max_bands())


def svt_workspace(P: int, B: int, device) -> torch.Tensor:
    n = int(lib().lrs_svt_workspace(P, B))
    return torch.zeros(n, dtype=torch.uint8, device=device)


def _svt_flags(warm, method, multi_wg=False, wide_tri=False, wide_mw=False):
    if method not in ("tri", "jacobi"):
        raise LrsError(f"unknown SVT eigensolver {method!r} (tri | jacobi)")
    return ((SVT_WARM if warm else 0) | (SVT_JACOBI if method == "jacobi" else 0) | (SVT_MULTI_WG if multi_wg else 0)
            | (SVT_WIDE_TRI if wide_tri else 0) | (SVT_WIDE_MW if wide_mw else 0))


SVT_CHAINS = ("tri", "tri-multi-wg", "jacobi", "wide-jacobi", "wide-tri")


def svt_plan(B: int, warm=False, method="tri", multi_wg=False, wide_tri=False, wide_mw=False) -> dict:
    """What the SVT calls do with B bands and these keywords of svt() (lrs_diag_svt_plan; host-only): the
    eigen chain (one of SVT_CHAINS), whether it warm-starts, whether the wide tridiagonal chain's reduction
    runs over many workgroups, and whether svt_gram() zeroes the state words / forms the warm-start products."""
    out = (ctypes.c_int32 * 8)()
    check(lib().lrs_diag_svt_plan(int(B), _svt_flags(warm, method, multi_wg, wide_tri, wide_mw), out), "lrs_diag_svt_plan")
    return dict(chain=SVT_CHAINS[out[0]], warm=bool(out[1]), mw_reduction=bool(out[2]), reset_state=bool(out[3]),
                warm_products=bool(out[4]))


def svt(X, L2, c2: float, tau: float, ws, U=None, s_out=None, warm=False, stream=None, method="tri",
        multi_wg=False, wide_tri=False, wide_mw=False):
    """U = SVT(X + c2*L2, tau) (main_LRS_PnP.py:118-124).  method 'tri': tridiagonal eigensolver
    with a certified Jacobi fallback (default); 'jacobi': Jacobi only (warm-startable).  multi_wg:
    the tridiagonal solver's eigenvalue / eigenvector / back-transformation phases over many
    workgroups (LRS_SVT_MULTI_WG, bit-identical).  Wide cubes (256 < B <= svt_max_bands()) take
    the Jacobi solver, warm-started when `warm` is set, unless wide_tri (LRS_SVT_WIDE_TRI) asks for
    their tridiagonal chain (state path 4, or 5 after its Jacobi fallback; method 'jacobi' wins;
    ignored at B <= 256); multi_wg is refused there.  wide_mw (LRS_SVT_WIDE_MW) beside wide_tri: that
    chain with its Householder reduction over many workgroups, one launch per column (state word 7 is
    then 1); ignored wherever the wide tridiagonal chain does not serve."""
    L = device_lib()
    dev(X, torch.float32, "X")
    if L2 is not None:
        dev(L2, torch.float32, "L2")
    P, B = X.shape
    if U is None:
        U = torch.empty_like(X)
    check(L.lrs_svt_f32(ptr(X), ptr(L2), float(c2), P, B, float(tau), ptr(U), ptr(s_out),
                        _svt_flags(warm, method, multi_wg, wide_tri, wide_mw), ptr(ws), ws.numel(), sptr(stream)),
          "lrs_svt_f32")
    return U


def svt_gram(X, L2, c2: float, ws, warm=False, stream=None, method="tri", wide_tri=False, wide_mw=False):
    """First half of svt(): fp64 Gram (+ the Jacobi warm-start product, which wide_tri does without,
    with or without wide_mw), multi-workgroup."""
    L = device_lib()
    P, B = X.shape
    check(L.lrs_svt_gram_f32(ptr(X), ptr(L2), float(c2), P, B,
                             _svt_flags(warm, method, wide_tri=wide_tri, wide_mw=wide_mw), ptr(ws), ws.numel(),
                             sptr(stream)), "lrs_svt_gram_f32")


def svt_gram_view(ws, P: int, B: int) -> torch.Tensor:
    """The fp64 Gram (Bp x Bp, Bp = B rounded up to even) that svt_gram() leaves in `ws`, as a
    tensor view: a slab-sharded caller all-reduces it in place before svt_finish()."""
    off, ld = outs(lib().lrs_svt_gram_offset, "lrs_svt_gram_offset", P, B, n=2, ctype=ctypes.c_int64)
    return ws[off: off + 8 * ld * ld].view(torch.float64).view(ld, ld)


def svt_finish(X, L2, c2: float, tau: float, ws, U, s_out=None, warm=False, stream=None, method="tri",
               multi_wg=False, wide_tri=False, wide_mw=False):
    """Second half of svt(): the eigensolver (one workgroup, or multi_wg; wide cubes: the Jacobi chain,
    or with wide_tri their tridiagonal chain, whose reduction wide_mw spreads over many workgroups), E,
    then U = Z - Z E."""
    L = device_lib()
    P, B = X.shape
    check(L.lrs_svt_finish_f32(ptr(X), ptr(L2), float(c2), P, B, float(tau), ptr(U), ptr(s_out),
                               _svt_flags(warm, method, multi_wg, wide_tri, wide_mw), ptr(ws), ws.numel(),
                               sptr(stream)), "lrs_svt_finish_f32")
    return U


def svt_state(ws, P: int, B: int):
    """The 32 state words of the last SVT call: V valid, V buffer, Jacobi rounds, sweeps, path (1 =
    tridiagonal, 2 = Jacobi fallback, 3 = Jacobi, 4 = wide tridiagonal, 5 = its Jacobi fallback), and of
    the wide tridiagonal chain its Newton-Schulz steps, certificate flag and word 7: 1 when the
    many-workgroup reduction (wide_mw) produced its triangle, 0 after the one-workgroup reduction; words
    8-31 are spare (diagnostics; syncs)."""
    out = (ctypes.c_int * 32)()
    check(device_lib().lrs_diag_svt_state(ptr(ws), P, B, ctypes.cast(out, ctypes.c_void_p)), "lrs_diag_svt_state")
    return list(out)


def svt_apply_only(X, L2, c2: float, ws, U, stream=None):
    """U = Z (I - E) alone, with the E the last solve left in `ws`: the apply kernel svt_finish()
    launches for this band count (diagnostics / timing)."""
    P, B = X.shape
    check(device_lib().lrs_diag_svt_apply(ptr(X), ptr(L2), float(c2), P, B, ptr(ws), ptr(U), sptr(stream)),
          "lrs_diag_svt_apply")
    return U


def tvprox_workspace(H: int, W: int, B: int, device) -> torch.Tensor:
    """Device workspace of tvprox() for an H x W image with B bands (lrs_tvprox_workspace: all five dual
    fields whatever the weights)."""
    n = int(lib().lrs_tvprox_workspace(int(H), int(W), int(B)))
    if n == 0:
        raise LrsError(f"lrs_tvprox_workspace: sizes not served (H {H}, W {W}, B {B}; positive, H*W*B < 2^31)")
    return torch.empty(n, dtype=torch.uint8, device=device)


def _cube_prox_args(X, L2, H: int, W: int, ws, U):
    """What tvprox() and nlmcube() check alike: X, L2 (or None) and ws on the device, P = H*W, and U (a new tensor
    when None) and L2 of X's shape.  Returns (B, U)."""
    dev(X, torch.float32, "X")
    if L2 is not None:
        dev(L2, torch.float32, "L2")
    dev(ws, torch.uint8, "ws")
    P, B = X.shape
    if P != H * W:
        raise LrsError(f"P = {P} != H*W = {H * W}")
    if U is None:
        U = torch.empty_like(X)
    dev(U, torch.float32, "U")
    if U.shape != X.shape or (L2 is not None and L2.shape != X.shape):
        raise LrsError(f"U {tuple(U.shape)} and L2 must have X's shape {tuple(X.shape)}")
    return B, U


def tvprox(X, L2, c2: float, H: int, W: int, ws, U=None, w_sp: float = 0.0, w_bd: float = 0.0, w_ss: float = 0.0,
           tau: float = 0.0, n_iter: int = 0, warm: bool = False, stats=None, stream=None):
    """U = argmin_u 1/2 ||u - Z||^2 + tau T(u), Z = X + c2*L2 (L2 may be None), T the spatial / band /
    spatial-spectral TV of the cube with weights w_sp / w_bd / w_ss: n_iter iterations of the fast gradient
    projection on the dual (lrs_tvprox_f32, include/lrspnp.h).  X (P, B) with P = H*W, p = i + H*j.
    warm: start from the dual variable the previous call left in `ws` (same sizes, same weights > 0).
    stats: a float64 device tensor of 2 elements that receives the primal objective and the duality gap.
    Returns U."""
    L = device_lib()
    B, U = _cube_prox_args(X, L2, H, W, ws, U)
    if stats is not None:
        dev(stats, torch.float64, "stats")
        if stats.numel() != 2:
            raise LrsError("stats must hold 2 doubles")
    check(L.lrs_tvprox_f32(ptr(X), ptr(L2), float(c2), int(H), int(W), B, float(w_sp), float(w_bd), float(w_ss),
                           float(tau), int(n_iter), TVPROX_WARM if warm else 0, ptr(U), ptr(stats), ptr(ws), ws.numel(),
                           sptr(stream)), "lrs_tvprox_f32")
    return U


def nlmcube_workspace(H: int, W: int, B: int, patch_size: int, patch_distance: int, device) -> torch.Tensor:
    """Device workspace of nlmcube() (lrs_nlmcube_workspace).  The one-launch kernel keeps everything in LDS, so
    the tensor has 0 elements."""
    n = int(lib().lrs_nlmcube_workspace(int(H), int(W), int(B), int(patch_size), int(patch_distance)))
    return torch.empty(n, dtype=torch.uint8, device=device)


def nlmcube(X, L2, c2: float, H: int, W: int, ws, U=None, patch_size: int = 7, patch_distance: int = 2, h: float = 0.05,
            sigma: float = 0.0, stream=None):
    """U = the spectral non-local means of Z = X + c2*L2 (L2 may be None): one weight per pixel pair from the
    patch distance over all bands, w = exp(-max(D / (B patch_size^2) - 2 sigma^2, 0) / h^2), applied to every
    band over the clipped search window |t| <= patch_distance (lrs_nlmcube_f32, include/lrspnp.h, which
    states the operator).  X (P, B) with P = H*W, p = y + H*x.  patch_size odd, at most 7; patch_distance at
    most 5.  Returns U."""
    L = device_lib()
    B, U = _cube_prox_args(X, L2, H, W, ws, U)
    check(L.lrs_nlmcube_f32(ptr(X), ptr(L2), float(c2), int(H), int(W), B, int(patch_size), int(patch_distance),
                            float(h), float(sigma), ptr(U), ptr(ws) if ws.numel() else None, ws.numel(), sptr(stream)),
          "lrs_nlmcube_f32")
    return U


def cube_quality_workspace(P: int, B: int, device) -> torch.Tensor:
    """Device workspace of cube_quality() for a P x B cube (lrs_cube_quality_workspace: the slab partials)."""
    n = int(lib().lrs_cube_quality_workspace(int(P), int(B)))
    if n == 0:
        raise LrsError(f"lrs_cube_quality_workspace: sizes not served (P {P}, B {B}; positive, P*B < 2^31)")
    return torch.empty(n, dtype=torch.uint8, device=device)


def cube_quality(X, C, region=None, ws=None, q=None, psnr_bands=None, stream=None):
    """q = (MPSNR, SAM in degrees, relative error, pixels counted for SAM) of X against the clean cube C, both
    (P, B) float32 unfolded, in one pass over both, in fp64 (lrs_cube_quality_f32, include/lrspnp.h, which
    states the definitions).  region: None (every entry counts) or uint8 (P, B), 1 = counted.  q: a float64
    device tensor of 4 elements; psnr_bands: None or one of B elements that receives the per-band PSNR.  No
    host sync.  Returns q."""
    L = device_lib()
    dev(X, torch.float32, "X")
    dev(C, torch.float32, "C")
    if X.dim() != 2 or C.shape != X.shape:
        raise LrsError(f"X {tuple(X.shape)} and C {tuple(C.shape)} must be the same (P, B)")
    P, B = X.shape
    if region is not None:
        dev(region, torch.uint8, "region")
        if region.shape != X.shape:
            raise LrsError(f"region {tuple(region.shape)} must have X's shape {tuple(X.shape)}")
    if ws is None:
        ws = cube_quality_workspace(P, B, X.device)
    dev(ws, torch.uint8, "ws")
    if q is None:
        q = torch.empty(4, dtype=torch.float64, device=X.device)
    dev(q, torch.float64, "q")
    if q.numel() != 4:
        raise LrsError("q must hold 4 doubles")
    if psnr_bands is not None:
        dev(psnr_bands, torch.float64, "psnr_bands")
        if psnr_bands.numel() != B:
            raise LrsError(f"psnr_bands must hold B = {B} doubles")
    check(L.lrs_cube_quality_f32(ptr(X), ptr(C), ptr(region), P, B, ptr(q), ptr(psnr_bands), ptr(ws), ws.numel(),
                                 sptr(stream)), "lrs_cube_quality_f32")
    return q


def keep_best(score, sign: int, iteration: int, src, dst, best, stream=None):
    """dst <- src and best <- (score, iteration) when score (a float64 device tensor, its first element) is
    better than best[0], decided on the device: sign +1 keeps the largest, -1 the smallest, strictly; a NaN
    score is never kept and a NaN best[0] (how best starts) is beaten by any other (lrs_keep_best_f32).  best:
    a float64 device tensor of 2 elements.  No host sync."""
    L = device_lib()
    dev(score, torch.float64, "score")
    dev(best, torch.float64, "best")
    dev(src, torch.float32, "src")
    dev(dst, torch.float32, "dst")
    if score.numel() < 1 or best.numel() != 2:
        raise LrsError("score must hold a double and best 2 doubles")
    if dst.numel() != src.numel():
        raise LrsError(f"dst has {dst.numel()} elements, src {src.numel()}")
    check(L.lrs_keep_best_f32(ptr(score), int(sign), int(iteration), ptr(src), ptr(dst), src.numel(), ptr(best),
                              sptr(stream)), "lrs_keep_best_f32")
    return best


def admm_update(X, L1, L2, Y, M, U, phi, bb, grid, gamma, mu1, mu2, norms=None, imout=None, stream=None):
    """In-place col2im + X update + dual updates (main_LRS_PnP.py:324-362)."""
    L = device_lib()
    P, B = X.shape
    n_pad = phi.shape[1]
    check(L.lrs_admm_update_f32(ptr(X), ptr(L1), ptr(L2), ptr(Y), ptr(M), ptr(U), ptr(phi), P, B, bb, n_pad,
                                ptr(grid["rstarts"]), ptr(grid["cstarts"]), grid["nbr"], ptr(grid["rlo"]),
                                ptr(grid["rhi"]), ptr(grid["clo"]), ptr(grid["chi"]), float(gamma), float(mu1),
                                float(mu2), ptr(norms), ptr(imout), sptr(stream)), "lrs_admm_update_f32")


def _image_out(X, H: int, W: int, out, Hf: int, Wf: int):
    """X (P, B) on the device with P = H*W, and the (B, Hf, Wf) image it goes into (a new tensor when out is
    None): the start of unfolded_to_image() and unfolded_to_frame().  Returns (B, out)."""
    dev(X, torch.float32, "X")
    P, B = X.shape
    if P != H * W:
        raise LrsError(f"P = {P} != H*W = {H * W}")
    return B, out if out is not None else torch.empty((B, Hf, Wf), dtype=torch.float32, device=X.device)


def unfolded_to_image(X, L, c: float, H: int, W: int, out=None, stream=None):
    """img[b][i][j] = X[i + H j][b] + c * L[...]   (…1-LiP.py:404 DIP_input layout)."""
    Ld = device_lib()
    B, out = _image_out(X, H, W, out, H, W)
    check(Ld.lrs_unfolded_to_image_f32(ptr(X), ptr(L), ctypes.c_float(c), H, W, B, ptr(out), sptr(stream)),
          "lrs_unfolded_to_image_f32")
    return out


def image_to_unfolded(img, H: int, W: int, out=None, stream=None):
    """X[i + H j][b] = img[b][i][j]   (…1-LiP.py:411 U layout)."""
    Ld = device_lib()
    dev(img, torch.float32, "img")
    B = img.numel() // (H * W)
    out = out if out is not None else torch.empty((H * W, B), dtype=torch.float32, device=img.device)
    check(Ld.lrs_image_to_unfolded_f32(ptr(img), H, W, B, ptr(out), sptr(stream)), "lrs_image_to_unfolded_f32")
    return out


def unfolded_to_frame(X, L, c: float, H: int, W: int, top: int, left: int, Hf: int, Wf: int, out=None, stream=None):
    """unfolded_to_image into rows top.., columns left.. of a (B, Hf, Wf) image whose frame is filled by
    reflection without repeating the edge (nn.ReflectionPad2d), in one pass (lrs_unfolded_to_frame_f32)."""
    Ld = device_lib()
    B, out = _image_out(X, H, W, out, Hf, Wf)
    if out.numel() != B * Hf * Wf:
        raise LrsError(f"out has {out.numel()} elements, not {B}x{Hf}x{Wf}")
    check(Ld.lrs_unfolded_to_frame_f32(ptr(X), ptr(L), ctypes.c_float(c), H, W, B, top, left, Hf, Wf, ptr(out),
                                       sptr(stream)), "lrs_unfolded_to_frame_f32")
    return out


def frame_to_unfolded(img, H: int, W: int, top: int, left: int, out=None, stream=None):
    """image_to_unfolded of the H x W image at (top, left) of the framed (B, Hf, Wf) img."""
    Ld = device_lib()
    dev(img, torch.float32, "img")
    if img.dim() != 3:
        raise LrsError(f"img {tuple(img.shape)} must be (B, Hf, Wf)")
    B, Hf, Wf = img.shape
    out = out if out is not None else torch.empty((H * W, B), dtype=torch.float32, device=img.device)
    if out.numel() != H * W * B:
        raise LrsError(f"out has {out.numel()} elements, not {H * W}x{B}")
    check(Ld.lrs_frame_to_unfolded_f32(ptr(img), H, W, B, top, left, Hf, Wf, ptr(out), sptr(stream)),
          "lrs_frame_to_unfolded_f32")
    return out


@contextlib.contextmanager
def _accumulating(stream, device, acc=None):
    """torch's allocations and arithmetic on `stream` (None: the current one) inside the block, and the fp64
    accumulator a kernel sums into: acc, or a new zeroed one."""
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        yield acc if acc is not None else torch.zeros(1, dtype=torch.float64, device=device)


def masked_mse(out, target, mask=None, want_grad: bool = True, stream=None, n_mean: int | None = None):
    """MSELoss(target*mask, out*mask) over the C x P elements of out (C, ...) and its gradient dL/dout
    (…1-LiP.py:234).  mask: None, P elements (every channel) or C*P elements (per band).
    n_mean: out holds its image inside a frame on which the mask is 0; the mean is over the image's n_mean
    elements instead of C*P (lrs_masked_mse_framed_f32).
    Returns (loss: float64 device scalar, gout or None)."""
    Ld = device_lib()
    dev(out, torch.float32, "out")
    dev(target, torch.float32, "target")
    if target.shape != out.shape or out.dim() < 2:
        raise LrsError(f"out {tuple(out.shape)} and target {tuple(target.shape)} must be the same (C, ...) shape")
    C = out.shape[0]
    P = out.numel() // C
    if mask is not None:
        dev(mask, torch.float32, "mask")
    mc = mask_channels(mask, C, P)
    gout = torch.empty_like(out) if want_grad else None
    with _accumulating(stream, out.device) as acc:
        if n_mean is None:
            check(Ld.lrs_masked_mse_cmask_f32(ptr(out), ptr(target), ptr(mask), mc, C, P, ptr(gout), ptr(acc),
                                              sptr(stream)), "lrs_masked_mse_cmask_f32")
            return acc / (C * P), gout
        check(Ld.lrs_masked_mse_framed_f32(ptr(out), ptr(target), ptr(mask), mc, C, P, int(n_mean), ptr(gout),
                                           ptr(acc), sptr(stream)), "lrs_masked_mse_framed_f32")
        return acc / int(n_mean), gout


def sstv(out, gout=None, loss_acc=None, frame=None, spatial: float = 0.0, band: float = 0.0, sstv: float = 0.0,
         eps: float = 0.0, n_mean: int | None = None, stream=None):
    """The smoothness term R of lrs_sstv_f32 on the image inside out (C, Hf, Wf): spatial TV, band TV and
    spatial-spectral TV with weights spatial / band / sstv, phi(d) = sqrt(d^2 + eps^2) (include/lrspnp.h).
    frame: (top, left, H, W) of the image, None = the whole of out.  n_mean: the N the sums are divided by
    (default the image's C*H*W).
    gout (C, Hf, Wf) += dR/do on the image (None: a new zero tensor, so the result is dR/do itself);
    loss_acc (float64, 1 element) += N * R (None: a new zero accumulator).
    Returns (loss_acc / N as a float64 device tensor, gout)."""
    Ld = device_lib()
    dev(out, torch.float32, "out")
    if out.dim() != 3:
        raise LrsError(f"out {tuple(out.shape)} must be (C, Hf, Wf)")
    C, Hf, Wf = out.shape
    top, left, H, W = (0, 0, Hf, Wf) if frame is None else (int(v) for v in frame)
    n = C * H * W if n_mean is None else int(n_mean)
    with _accumulating(stream, out.device, loss_acc) as loss_acc:
        if gout is None:
            gout = torch.zeros_like(out)
        dev(gout, torch.float32, "gout")
        dev(loss_acc, torch.float64, "loss_acc")
        if gout.shape != out.shape or loss_acc.numel() != 1:
            raise LrsError(f"gout {tuple(gout.shape)} must have out's shape {tuple(out.shape)} and loss_acc one element")
        check(Ld.lrs_sstv_f32(ptr(out), C, Hf, Wf, top, left, H, W, ctypes.c_float(spatial), ctypes.c_float(band),
                              ctypes.c_float(sstv), ctypes.c_float(eps), n, ptr(gout), ptr(loss_acc), sptr(stream)),
              "lrs_sstv_f32")
        return loss_acc / n, gout

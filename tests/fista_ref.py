"""Float32 numpy restatement of the masked sparse-coding iteration of include/lrspnp.h, plain
(lrs_ista_opts.accel = 0, the reference's ista()) and accelerated (LRS_ISTA_ACCEL_FISTA), the
reference of test_fista_ref.py and test_gpu_ista_accel.py.

Start with x_0 (zero or `x0`), z_1 = x_0, t_1 = 1.  For k = 1..Nit:
    x_k     = prox(z_k + D^T(m .* (y - D z_k)) / alpha)
    t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2
    beta_k  = (t_k - 1) / t_{k+1}
    z_{k+1} = x_k + beta_k (x_k - x_{k-1})
and the result is x_Nit with Phi = D x_Nit.  With accel off beta is 0 and this is oracle.ista_batch.

Every iterate is float32.  The two products accumulate in float64 and round once to float32, where
oracle/lrs_oracle.c rounds them (torch.mm's float32 result); the subtraction, the quotient by alpha,
the sum and the momentum step are float32 operations; t and beta are float64, beta rounded once to
float32.  The prox is the oracle's own: oracle.nlm_col, oracle.nlm_matlab_col, or the soft threshold as
lrs_oracle.c writes it.
"""
import numpy as np

from oracle import oracle as O


def prox_rows(G, thr, prox):
    """The prox of every row of G (nb, K) float32 with its own threshold thr[j]."""
    G = np.ascontiguousarray(G, np.float32)
    if prox == O.PROX_SOFT:
        T = np.asarray(thr, np.float64).astype(np.float32)[:, None]
        t = np.maximum(np.abs(G) - T, np.float32(0))
        return np.where(G > 0, t, np.where(G < 0, -t, np.float32(0))).astype(np.float32)
    f = O.nlm_matlab_col if prox == O.PROX_NLM_MATLAB else O.nlm_col
    return np.stack([f(G[j], float(thr[j])) for j in range(G.shape[0])])


def betas(Nit):
    """beta_1 .. beta_Nit as float32 (t in float64)."""
    out, t = np.empty(int(Nit), np.float32), 1.0
    for k in range(int(Nit)):
        tn = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
        out[k] = np.float32((t - 1.0) / tn)
        t = tn
    return out


def ista(Yb, obs, D, alpha, thr, Nit, prox=O.PROX_NLM, accel=False, x0=None):
    """(X (nb, K), PHI (nb, n)) float32 for blocks Yb (nb, n), masks obs (nb, n), D (n, K)."""
    Y = np.ascontiguousarray(Yb, np.float32)
    m = np.asarray(obs) != 0
    D = np.ascontiguousarray(D, np.float32)
    D64 = D.astype(np.float64)
    a = np.asarray(alpha, np.float32)[:, None]
    nb, K = Y.shape[0], D.shape[1]
    X = np.zeros((nb, K), np.float32) if x0 is None else np.array(x0, np.float32)
    Z, Xprev = X.copy(), X.copy()
    beta = betas(Nit)
    for k in range(int(Nit)):
        R = (Z.astype(np.float64) @ D64.T).astype(np.float32)
        r = np.where(m, Y - R, np.float32(0)).astype(np.float32)
        q = (r.astype(np.float64) @ D64).astype(np.float32) / a
        X = prox_rows(Z + q, thr, prox)
        if accel and k + 1 < int(Nit):
            Z = (X + beta[k] * (X - Xprev)).astype(np.float32)
            Xprev = X
        else:
            Z = X
    PHI = (X.astype(np.float64) @ D64.T).astype(np.float32)
    return X, PHI


def lasso_objective(Yb, obs, D, X, lam):
    """||m .* (y - D x)||^2 + lam ||x||_1 per block, float64."""
    m = np.asarray(obs) != 0
    R = np.where(m, np.asarray(Yb, np.float64) - np.asarray(X, np.float64) @ np.asarray(D, np.float64).T, 0.0)
    return np.sum(R * R, axis=1) + float(lam) * np.sum(np.abs(np.asarray(X, np.float64)), axis=1)


def rand_blocks(rng, nb, n, miss_frac, scale=0.3):
    """The data of test_gpu_kernels.py's ISTA tests: `miss_frac` missing, block 0 fully observed,
    block 1 with its first half masked."""
    Yb = (rng.standard_normal((nb, n)) * scale).astype(np.float32)
    obs = (rng.random((nb, n)) > miss_frac).astype(np.uint8)
    obs[0, :] = 1
    if nb > 2:
        obs[1, : n // 2] = 0
    Yb[obs == 0] = 0.0
    return Yb, obs


def case(bb, nb, variant, K, seed, dict_seed=3):
    """(D, Yb, obs, alpha, thr, prox) of one (bb, nb, variant, K) shape, as test_ista_kernel_vs_oracle."""
    from lrspnp.data import synthetic_dictionary
    rng = np.random.default_rng(seed)
    n = bb * bb
    D = synthetic_dictionary(n, K, seed=dict_seed)
    Yb, obs = rand_blocks(rng, nb, n, 0.2)
    alpha = np.empty(nb, np.float32)
    thr = np.empty(nb, np.float64)
    for j in range(nb):
        alpha[j], thr[j] = O.ista_alpha_h(D[obs[j].astype(bool)], 0.1, variant)
    prox = {"soft": O.PROX_SOFT, "matlab": O.PROX_NLM_MATLAB}.get(variant, O.PROX_NLM)
    return D, Yb, obs, alpha, thr, prox

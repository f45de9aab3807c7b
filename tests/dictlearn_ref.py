"""Plain-numpy checker of masked dictionary learning (the reference of test_dictlearn.py and
test_gpu_dictlearn.py).  Every function takes `dtype`: np.float64 (the reference) or np.float32 (the
same arithmetic in single precision, to measure what rounding alone does to the result).

* ISTA with the soft threshold as ista.m:15-23 and oracle/lrs_oracle.c state it: per block, H = the
  observed rows of D, alpha = ||H||_2^2, T = lambda / (2 alpha), x = 0, then Nit times
  x = soft(x + H^T (y - H x) / alpha, T).  A block with nothing observed takes alpha = T = 1.
* The dictionary step (Yaghoobi, Blumensath, Davies, with the mask inside the residual):
  H = A^T A, c = max_k sum_l |H_kl|, then n_inner times R = m .* (Y - A D^T), obj = 1/2 ||R||_F^2,
  G = R^T A, u_k = d_k + g_k / c, d_k = u_k / max(1, ||u_k||); g_k = 0 where H_kk = 0; c = 0 leaves D.

Layouts as the kernels': Y, obs (nb, n), A (nb, K), D (n, K).
"""
import numpy as np


def ista_alpha_soft(D, obs, lam, dtype=np.float64):
    """(alpha, T, inv) per block, computed once per distinct observation pattern."""
    D = np.asarray(D, dtype)
    packed = np.packbits(np.asarray(obs, np.uint8) != 0, axis=1)
    uniq, inv = np.unique(packed, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    n = D.shape[0]
    alpha_p = np.ones(uniq.shape[0], dtype)
    thr_p = np.ones(uniq.shape[0], dtype)
    for p in range(uniq.shape[0]):
        rows = np.unpackbits(uniq[p])[:n].astype(bool)
        if rows.any():
            a = dtype(np.linalg.norm(D[rows], 2)) ** 2
            alpha_p[p] = a
            thr_p[p] = dtype(lam) / (dtype(2) * a)
    return alpha_p[inv], thr_p[inv]


def ista_soft(Y, obs, D, alpha, thr, Nit, x0=None, dtype=np.float64):
    """All blocks at once; x0 (nb, K) continues from given coefficients."""
    Y, D = np.asarray(Y, dtype), np.asarray(D, dtype)
    m = (np.asarray(obs) != 0).astype(dtype)
    a, t = np.asarray(alpha, dtype)[:, None], np.asarray(thr, dtype)[:, None]
    X = np.zeros((Y.shape[0], D.shape[1]), dtype) if x0 is None else np.array(x0, dtype)
    for _ in range(int(Nit)):
        R = m * (Y - X @ D.T)
        G = X + (R @ D) / a
        X = np.sign(G) * np.maximum(np.abs(G) - t, dtype(0))
    return X


def dict_stats(A, dtype=np.float64):
    A = np.asarray(A, dtype)
    H = A.T @ A
    c = float(np.max(np.sum(np.abs(H.astype(np.float64)), axis=1))) if H.size else 0.0
    return H, c


def dict_step(Y, obs, A, D, n_inner, c=None, dtype=np.float64):
    """n_inner iterations; returns (D, obj) with obj (n_inner + 1,) float64: the objective before each
    iteration and after the last.  obj and the column norms accumulate in float64 in either mode."""
    Y, A, D = np.asarray(Y, dtype), np.asarray(A, dtype), np.array(D, dtype)
    m = (np.asarray(obs) != 0).astype(dtype)
    if c is None:
        c = dict_stats(A, dtype)[1]
    used = np.any(A != 0, axis=0)
    obj = np.empty(int(n_inner) + 1, np.float64)

    def resid(Dc):
        R = m * (Y - A @ Dc.T)
        return R, 0.5 * float(np.sum(R.astype(np.float64) ** 2))

    for it in range(int(n_inner)):
        R, obj[it] = resid(D)
        if c > 0:
            G = R.T @ A
            G[:, ~used] = 0
            U = D + G / dtype(c)
            nrm = np.sqrt(np.sum(U.astype(np.float64) ** 2, axis=0))
            D = (U / np.maximum(nrm, 1.0).astype(dtype)).astype(dtype)
    obj[int(n_inner)] = resid(D)[1]
    return D, obj


def normalise(D, dtype=np.float64):
    D = np.array(D, dtype)
    nrm = np.sqrt(np.sum(D.astype(np.float64) ** 2, axis=0))
    nrm[nrm == 0] = 1.0
    return (D / nrm.astype(dtype)).astype(dtype)


def learn(Y, obs, D0, lam, Nit, rounds, n_inner, warm=True, normalise_end=True, dtype=np.float64):
    """The alternating minimisation; returns (D, history (rounds, n_inner + 1) float64, A)."""
    D = np.array(D0, dtype)
    A = None
    hist = np.empty((int(rounds), int(n_inner) + 1), np.float64)
    for r in range(int(rounds)):
        alpha, thr = ista_alpha_soft(D, obs, lam, dtype)
        A = ista_soft(Y, obs, D, alpha, thr, Nit, x0=A if (warm and r > 0) else None, dtype=dtype)
        D, hist[r] = dict_step(Y, obs, A, D, n_inner, dtype=dtype)
    if normalise_end:
        D = normalise(D, dtype)
    return D, hist, A


def coded_objective(Y, obs, D, lam, Nit, dtype=np.float64):
    """1/2 ||m .* (Y - A D^T)||^2 with A = the ISTA codes of Y on D from zero."""
    alpha, thr = ista_alpha_soft(D, obs, lam, dtype)
    A = ista_soft(Y, obs, D, alpha, thr, Nit, dtype=dtype)
    m = (np.asarray(obs) != 0)
    R = m * (np.asarray(Y, np.float64) - A.astype(np.float64) @ np.asarray(D, np.float64).T)
    return 0.5 * float(np.sum(R ** 2))


def planted_problem(n=64, K=32, nb=2000, sparsity=3, masked=0.10, noise=0.01, seed=0):
    """Data from a seeded unit-norm D* with `sparsity`-sparse codes, `masked` of the rows of each
    block unobserved, Gaussian noise.  Returns (Y float32 with zeros at missing entries, obs u8,
    D* float64, D0 float32: K seeded distinct blocks, missing entries at the observed mean, unit norm)."""
    rng = np.random.default_rng(seed)
    Ds = rng.standard_normal((n, K))
    Ds /= np.linalg.norm(Ds, axis=0, keepdims=True)
    A = np.zeros((nb, K))
    for j in range(nb):
        idx = rng.choice(K, sparsity, replace=False)
        A[j, idx] = rng.uniform(0.5, 1.5, sparsity) * rng.choice([-1.0, 1.0], sparsity)
    Y = A @ Ds.T + noise * rng.standard_normal((nb, n))
    obs = np.ones((nb, n), np.uint8)
    nm = int(round(masked * n))
    for j in range(nb):
        obs[j, rng.choice(n, nm, replace=False)] = 0
    Y = (Y * obs).astype(np.float32)
    pick = np.sort(rng.choice(nb, K, replace=False))
    D0 = np.empty((n, K))
    for k, j in enumerate(pick):
        o = obs[j] != 0
        a = np.where(o, Y[j].astype(np.float64), Y[j][o].mean())
        D0[:, k] = a / np.linalg.norm(a)
    return Y, obs, Ds, D0.astype(np.float32)


def recovered(D, Dstar, thresh=0.99):
    """Number of planted atoms d* with max_k |<d_k, d*>| > thresh (D's columns normalised first)."""
    Dn = normalise(D)
    return int(np.sum(np.max(np.abs(Dn.T @ np.asarray(Dstar, np.float64)), axis=0) > thresh))


def update_problem(n, n_pad, K, nb, seed):
    """Inputs of one dictionary step at the kernels' layouts: Yb, obs (nb, n_pad), coefs (nb, K) about
    10 % dense with one all-zero column, D (n, K) unit-norm.  Masks mix fully observed blocks, blocks
    with whole rows missing, random patterns and one block with nothing observed; the pad columns
    i >= n hold obs = 1 and large values on purpose: they must never contribute."""
    rng = np.random.default_rng(seed)
    D = rng.standard_normal((n, K))
    D /= np.linalg.norm(D, axis=0, keepdims=True)
    A = rng.standard_normal((nb, K)) * (rng.random((nb, K)) < 0.1)
    A[:, K // 3] = 0
    Y = A @ D.T + 0.05 * rng.standard_normal((nb, n))
    obs = np.ones((nb, n), np.uint8)
    bb = int(round(np.sqrt(n)))
    for j in range(nb):
        kind = j % 3
        if kind == 1 and bb * bb == n:                      # whole rows of the bb x bb block missing
            blk = np.ones((bb, bb), np.uint8)
            blk[rng.choice(bb, max(1, bb // 5), replace=False), :] = 0
            obs[j] = blk.reshape(-1, order="F")
        elif kind == 1:
            obs[j, rng.choice(n, n // 5, replace=False)] = 0
        elif kind == 2:
            obs[j] = rng.random(n) > 0.2
    obs[nb // 2] = 0                                        # nothing observed
    Yb = np.full((nb, n_pad), 1e3, np.float32)
    Yb[:, :n] = (Y * obs).astype(np.float32)
    ob = np.ones((nb, n_pad), np.uint8)
    ob[:, :n] = obs
    return Yb, ob, np.ascontiguousarray(A.astype(np.float32)), np.ascontiguousarray(D.astype(np.float32))

"""CPU fp64 model of the step-size kernel (csrc/alpha.hip: k_alpha, spec2 / soft path) and the operand
sets of its tests.

Imported by tests/test_alpha_emu.py (CPU: the model against the fp64 SVD, and the proof that the hard
inputs are hard for a capped Lanczos run and easy for the reference) and tests/test_gpu_alpha.py (the
kernel against the fp64 SVD on the same matrices).  The model chooses inputs and explains failures; it
is never the expected value of a GPU test.

The model follows the kernel statement by statement: the observed rows of D, the smaller of
D_m D_m^T (m_obs <= K) and D_m^T D_m, the start vector 1 + 0.5 sin(0.7 i + 0.3), the three-term step
with a_k taken before the subtraction, classical Gram-Schmidt against every stored vector applied
twice, the b_k > 1e-13 |a_k| breakdown test, the step cap, the Gershgorin bracket and Sturm bisection
for the top eigenvalue of the tridiagonal, and alpha = float32(sqrt(lambda))^2.  With cycles > 1 it
also follows the restart: the top eigenvector of the tridiagonal by a twisted factorisation at the
upper end of the bisection bracket, the residual bound b_k |s_k| against tol * lambda, and a new run
from the Ritz vector.  cycles = 1 is the kernel as it was before the restart.  What the model does not
reproduce is the order of the fp64 sums inside a product (relative 1e-16, nine decades below a float32
ulp).
"""
import math

import numpy as np

LANCZOS_MAX = 128          # kLanczosMax
CYCLES = 16                # kAlphaCycles
TOL = 2.0 ** -28           # kAlphaTol


def ulp32(a, b):
    """Distance of two float32 values in units of the last place (same sign, finite)."""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def alpha_ref(H):
    """alpha = float32(sigma_max)^2 with sigma_max from the fp64 SVD of the float32 H; 1.0 for no rows."""
    H = np.asarray(H)
    assert H.dtype == np.float32
    if H.shape[0] == 0:
        return np.float32(1.0)
    s = np.linalg.svd(H.astype(np.float64), compute_uv=False)[0]
    a = np.float32(s) ** 2
    assert a.dtype == np.float32
    return a if a > 0 else np.float32(1.0)


def thr_ref(alpha, lambda_ista, variant):
    """The float32 expressions of oracle.ista_alpha_h for the threshold that goes with alpha."""
    T = np.float32(lambda_ista) / (np.float32(2) * np.float32(alpha))
    return float(np.float32(T * np.float32(0.1)) if variant in ("spec2", "matlab") else np.float32(T))


# ---- the tridiagonal ---------------------------------------------------------------------------------

def _count_greater(al, be, k, x):
    neg = 0
    d = 1.0
    for i in range(k):
        d = (al[i] - x) - (be[i - 1] * be[i - 1] / d if i > 0 else 0.0)
        if d == 0.0:
            d = -1e-300
        if d < 0.0:
            neg += 1
    return k - neg


def tri_top(al, be, k):
    """(lmax, hi): the kernel's bisection for the top eigenvalue of the k x k tridiagonal, and the upper
    end of its last bracket."""
    lo, hi = 1e300, -1e300
    for i in range(k):
        r = (abs(be[i - 1]) if i > 0 else 0.0) + (abs(be[i]) if i + 1 < k else 0.0)
        lo = min(lo, al[i] - r)
        hi = max(hi, al[i] + r)
    for _ in range(200):
        if not hi - lo > 0.0:
            break
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if _count_greater(al, be, k, mid) >= 1:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi), hi


def tri_vec(al, be, k, x):
    """Unit eigenvector of the tridiagonal for its eigenvalue next to x, by the twisted factorisation
    of T - x I (x at or above the top eigenvalue: every pivot is negative)."""
    dp = np.empty(k)
    dm = np.empty(k)
    lp = np.zeros(k)
    um = np.zeros(k)

    def piv(d):
        return d if d != 0.0 else -1e-300

    dp[0] = piv(al[0] - x)
    for i in range(1, k):
        lp[i - 1] = be[i - 1] / dp[i - 1]
        dp[i] = piv((al[i] - x) - be[i - 1] * lp[i - 1])
    dm[k - 1] = piv(al[k - 1] - x)
    for i in range(k - 2, -1, -1):
        um[i] = be[i] / dm[i + 1]
        dm[i] = piv((al[i] - x) - be[i] * um[i])
    r, g = 0, math.inf
    for i in range(k):
        gi = abs(dp[i] + dm[i] - (al[i] - x))
        if gi < g:
            r, g = i, gi
    z = np.zeros(k)
    z[r] = 1.0
    for i in range(r - 1, -1, -1):
        z[i] = -lp[i] * z[i + 1]
    for i in range(r, k - 1):
        z[i + 1] = -um[i] * z[i]
    return z / math.sqrt(float(np.sum(z * z)))


# ---- the kernel --------------------------------------------------------------------------------------

def alpha_model(D, obs, cap=LANCZOS_MAX, cycles=CYCLES, tol=TOL, info=None):
    """float32 alpha of the kernel's spec2 path for dictionary D (n, K) float32 and one observation
    pattern obs (n,) of bytes.  cap: Lanczos steps per run (None: min(m_obs, K), the complete run);
    cycles: runs at the most; info: a dict that receives steps, cycles, lmax and the last residual."""
    D = np.asarray(D)
    assert D.dtype == np.float32 and D.ndim == 2
    n, K = D.shape
    rows = np.flatnonzero(np.asarray(obs)[:n])
    m_obs = rows.size
    Dm = D[rows].astype(np.float64)
    small = m_obs <= K
    m = m_obs if small else K
    lmax, steps, cyc, resid = 0.0, 0, 0, 0.0
    if m > 0:
        A = (lambda v: Dm @ (Dm.T @ v)) if small else (lambda v: Dm.T @ (Dm @ v))
        kmax = m if cap is None else min(m, cap)
        i = np.arange(m, dtype=np.float64)
        q = 1.0 + 0.5 * np.sin(0.7 * i + 0.3)
        q = q / math.sqrt(float(np.sum(q * q)))
        while True:
            cyc += 1
            qprev = np.zeros(m)
            beta_prev = 0.0
            Q = np.zeros((kmax, m))
            al = np.zeros(kmax)
            be = np.zeros(kmax)
            broke = False
            k = 0
            while k < kmax:
                Q[k] = q
                w = A(q)
                a_k = float(np.sum(q * w))
                w = w - a_k * q - beta_prev * qprev
                for _ in range(2):
                    w = w - Q[:k + 1].T @ (Q[:k + 1] @ w)
                b_k = math.sqrt(float(np.sum(w * w)))
                al[k], be[k] = a_k, b_k
                steps += 1
                if not b_k > 1e-13 * abs(a_k):
                    broke = True
                    k += 1
                    break
                if k + 1 == kmax:
                    k += 1
                    break
                qprev, q, beta_prev = q, w / b_k, b_k
                k += 1
            lmax, hi = tri_top(al, be, k)
            if broke or k == m or cycles <= 1:
                break
            s = tri_vec(al, be, k, hi)
            resid = be[k - 1] * abs(s[k - 1])
            if resid <= tol * lmax or cyc == cycles:
                break
            q = Q[:k].T @ s
            q = q / math.sqrt(float(np.sum(q * q)))
    if info is not None:
        info.update(steps=steps, cycles=cyc, lmax=lmax, resid=resid, m=m)
    sigma = np.float32(math.sqrt(max(lmax, 0.0)))
    a = sigma * sigma
    return a if a > 0 else np.float32(1.0)


# ---- inputs ------------------------------------------------------------------------------------------

SPECTRA = ("packed_quad", "packed_lin", "top_pair", "repeated5", "all_equal", "rank3")
HARD_SHAPES = ((300, 256), (600, 512))


def spectrum(name, r):
    i = np.arange(r, dtype=np.float64)
    tail = np.linspace(0.9, 0.1, r)
    if name == "packed_quad":                       # a smoothly packed top
        return 1.0 - 1e-2 * (i / r) ** 2
    if name == "packed_lin":
        return 1.0 - 1e-4 * i / r
    if name == "top_pair":                          # a top pair split by 1e-7 over a spread tail
        return np.concatenate(([1.0, 1.0 - 1e-7], tail[2:]))
    if name == "repeated5":                         # an exactly repeated top value, multiplicity 5
        return np.concatenate((np.ones(5), tail[5:]))
    if name == "rank3":
        return np.concatenate(([1.0, 0.7, 0.4], np.zeros(r - 3)))
    raise ValueError(name)


def _orth(rng, rows, cols):
    q, _ = np.linalg.qr(rng.standard_normal((rows, cols)))
    return q


def _hadamard(k):
    h = np.ones((1, 1))
    while h.shape[0] < k:
        h = np.block([[h, h], [h, -h]])
    assert h.shape[0] == k
    return h


def hard_matrix(name, n, K, seed=0):
    """float32 H (n, K), n > K, with the named singular values up to float32 rounding of its entries.
    all_equal is exact instead: a Hadamard matrix times a power of two between zero rows, so that
    H^T H is a multiple of the identity in fp64 too and the Lanczos run breaks down at its first step."""
    assert n > K
    rng = np.random.default_rng([seed, n, K, SPECTRA.index(name)])
    if name == "all_equal":
        H = np.zeros((n, K))
        H[np.sort(rng.permutation(n)[:K])] = _hadamard(K) * 2.0 ** -(int(math.log2(K)) // 2)
        return H.astype(np.float32)
    s = spectrum(name, K)
    return ((_orth(rng, n, K) * s) @ _orth(rng, K, K).T).astype(np.float32)


def random_dictionary(n, K, seed):
    """Unit-column Gaussian float32 dictionary (n, K)."""
    rng = np.random.default_rng([seed, n, K])
    D = rng.standard_normal((n, K))
    return (D / np.linalg.norm(D, axis=0)).astype(np.float32)


def mask_with(n, m_obs, seed):
    """One observation pattern (n,) of bytes with exactly m_obs ones."""
    rng = np.random.default_rng([seed, n, m_obs])
    o = np.zeros(n, np.uint8)
    o[rng.permutation(n)[:m_obs]] = 1
    return o
